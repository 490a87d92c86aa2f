"""-m gpu: SDE sampling inside the engine (lt_sample_sde, csrc/sde.hip).

* the fused step kernels (lt_op_sde_step) against the host loop's own tensor expressions run by torch on the same device (tests/sde_torch.py):
  every output word equal;
* Sampler.sample_sde with the engine path against the same sampler on its host loop (use_engine = False) through the same engine-backed
  model under the same seed: every returned state equal, at bf16 and fp32 states, with half the model evaluations;
* the engine trajectory against the UNMODIFIED reference sampler (tests/golden/sde_imagenet_tiny.npz) under the standing rule
  rel_l2(engine, ref fp32) <= 1.5 x min(rel_l2 of the reference's own bf16 realisations) at every stored step;
* the refusals of lt_sample_sde by name."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import integrators as I
from lumina_t2x_amd.transport import path
from oracle import synth

import sde_torch as ST
from gpu_util import P, lib, rel_l2, stream

pytestmark = pytest.mark.gpu

FORMS = ("SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing")


# ---- how PyTorch treats the loop's scalar operands on this device: what csrc/sde.hip and sde_table assume ------------------------------
def test_scalar_operands_of_the_loop_multiply_in_fp32_and_a_device_scalar_divides_in_the_state_dtype():
    torch.manual_seed(0)
    x = torch.randn(4096, device="cuda").to(torch.bfloat16)
    dt = torch.linspace(0.0, 0.96, 250)[1] - torch.linspace(0.0, 0.96, 250)[0]  # a 0-dim CPU fp32 tensor, like sde.dt
    assert float(dt) != float(dt.to(torch.bfloat16))
    for s in (dt, torch.sqrt(dt), 0.5 * dt):
        in_fp32 = (x.float() * float(s)).to(torch.bfloat16)
        cast_first = (x.float() * float(s.to(torch.bfloat16))).to(torch.bfloat16)
        assert not torch.equal(in_fp32, cast_first)
        assert torch.equal(x * s, in_fp32) and torch.equal(s * x, in_fp32)
    h = 0.04  # a Python float, like last_step_size
    assert torch.equal(x * h, (x.float() * float(torch.tensor(h, dtype=torch.float32))).to(torch.bfloat16))
    t = torch.tensor([0.3, 0.5], device="cuda").to(torch.bfloat16)
    assert torch.equal(t + dt, (t.float() + float(dt)).to(torch.bfloat16))
    a = torch.tensor(0.9573, device="cuda")  # a 0-dim DEVICE fp32 tensor, like compute_alpha_t(t)[0][0] of the Tweedie rule
    assert float(a) != float(a.to(torch.bfloat16))
    assert torch.equal(x / a, (x.float() / a.to(torch.bfloat16).float()).to(torch.bfloat16))
    assert (x / a).dtype == torch.bfloat16 and (x * torch.ones(1, device="cuda")).dtype == torch.float32


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
def _records(form, dtype):
    """stage records of a Heun step and a last-step record from the plan's own functions (Linear path away from t = 0, norm 0.7)"""
    plan = path.ICPlan()
    t = torch.linspace(0.07, 0.93, 6)
    like = torch.zeros(1, dtype=dtype, device="cuda")
    steps, last = I.sde_table(plan, form, 0.7, t, t[1] - t[0], "Heun", like, "Tweedie", 0.04, 0.93)
    return steps[4], steps[5], last


def _op(op, x, v, w, k1, xp, rec, out_dtype, two_out=False):
    out = torch.full(x.shape, float("nan"), dtype=out_dtype, device=x.device)
    out2 = torch.full(x.shape, float("nan"), dtype=x.dtype, device=x.device) if two_out else None
    recf = (C.c_float * _lib.LT_SDE_REC)(*[float(u) for u in rec])
    rc = lib().lt_op_sde_step(ST.OPS[op], P(x), P(v), P(w), P(k1), P(xp), P(out), P(out2), recf, x.numel(),
                              _lib.LT_BF16 if x.dtype == torch.bfloat16 else _lib.LT_F32, stream())
    _lib.check(rc, f"lt_op_sde_step({op})")
    return out, out2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("form", FORMS)
def test_step_kernels_equal_the_torch_expressions_word_for_word(form, dtype):
    rec1, rec2, last = _records(form, dtype)
    g = torch.Generator(device="cuda").manual_seed(11)
    # whole groups only, a tail behind whole groups, fewer elements than one group, one element; a second round on buffers that start one
    # element into their allocation (not 16-byte aligned: the one-element-per-thread form)
    for n in (2 * 4 * 16 * 16, 8 * 1024 + 5, 4099, 7, 3, 1):
        for shift in (0, 1):
            x, v, w, k1, xp = ((torch.randn(n + shift, generator=g, device="cuda") * s).to(dtype)[shift:] for s in (1.0, 1.5, 1.0, 2.0, 1.0))
            assert x.data_ptr() % 16 == (0 if shift == 0 else x.element_size())
            x4 = lambda u: u.reshape(1, 1, 1, -1)  # noqa: E731
            c1, c2 = ST.Stage(rec1, x), ST.Stage(rec2, x)
            tag = (form, dtype, n, shift)
            got, _ = _op("euler", x, v, w, None, None, rec1, dtype)
            assert torch.equal(got, ST.euler(x4(x), x4(v), x4(w), c1).reshape(-1)), ("euler",) + tag
            got, _ = _op("heun_xhat", x, None, w, None, None, rec1, dtype)
            assert torch.equal(got, ST.heun_xhat(x4(x), x4(w), c1).reshape(-1)), ("heun_xhat",) + tag
            got, got2 = _op("heun_k1", x, v, None, None, None, rec1, dtype, two_out=True)
            want, want2 = ST.heun_k1(x4(x), x4(v), c1)
            assert torch.equal(got, want.reshape(-1)) and torch.equal(got2, want2.reshape(-1)), ("heun_k1",) + tag
            got, _ = _op("heun_out", x, v, None, k1, xp, rec2, dtype)
            assert torch.equal(got, ST.heun_out(x4(x), x4(v), x4(k1), x4(xp), c2).reshape(-1)), ("heun_out",) + tag
            for rule in ("Mean", "Tweedie", "Euler"):
                want = ST.last(x4(x), x4(v), last, rule).reshape(-1)
                assert want.dtype == (dtype if rule == "Euler" else torch.float32)
                got, _ = _op(rule, x, v, None, None, None, last, want.dtype)
                assert torch.equal(got, want), (rule,) + tag


# ---- loop ----------------------------------------------------------------------------------------------------------------------------
def _model(golden_dir, family):
    name, ctor = {"imagenet": ("imagenet_tiny", models.imagenet.DiT_Llama), "next": ("nextdit_tiny", models.NextDiT),
                  "flag": ("flag_tiny", models.flag_dit.DiT_Llama), "moe_time": ("moe_time_tiny", models.moe.DiT_Llama_TimeMoE)}[family]
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    m = ctor(**cfg.ctor_kwargs())
    m.load_state_dict(synth.synth_state_dict(cfg, seed=int(g["seed_w"])), strict=True)
    m = m.eval().to("cuda", torch.bfloat16)
    z = torch.from_numpy(g["z"])
    if cfg.has_text:
        kw = dict(cap_feats=torch.from_numpy(g["cap"]).to("cuda", torch.bfloat16), cap_mask=torch.from_numpy(g["mask"]).cuda(), cfg_scale=4.0,
                  proportional_attn=True, base_seqlen=16)
    else:
        kw = dict(y=torch.from_numpy(g["y"]).cuda(), cfg_scale=4.0)
    return m, z, kw


LOOP_CASES = [
    # family, path, method, form, last step
    ("imagenet", "Linear", "Euler", "sigma", "Mean"),
    ("imagenet", "VP", "Heun", "SBDM", "Tweedie"),
    ("imagenet", "GVP", "Heun", "decreasing", None),
    ("next", "Linear", "Euler", "linear", "Euler"),
    ("next", "Linear", "Heun", "sigma", "Tweedie"),
    ("flag", "Linear", "Heun", "inccreasing-decreasing", "Mean"),
    ("flag", "VP", "Euler", "SBDM", "Tweedie"),
    ("moe_time", "Linear", "Euler", "sigma", "Mean"),
    ("moe_time", "Linear", "Heun", "linear", "Euler"),
]


@pytest.mark.parametrize("state_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("family,ptype,method,form,last_step", LOOP_CASES)
def test_engine_loop_equals_the_host_loop_state_for_state_with_half_the_evaluations(golden_dir, family, ptype, method, form, last_step, state_dtype):
    model, z, kw = _model(golden_dir, family)
    z = z.to("cuda", state_dtype)
    n = 6
    fn = Sampler(create_transport(ptype, "velocity", None, None, None)).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=0.8,
                                                                                   last_step=last_step, last_step_size=0.04, num_steps=n)
    assert fn.solver.use_engine is True
    torch.manual_seed(77)
    got = fn(z, model.forward_with_cfg, **kw)
    stages = 2 if method == "Heun" else 1
    nfe = (n - 1) * stages + (last_step is not None)
    assert model._engine.last_nfe() == nfe

    calls = []

    class Counted:  # the same bound method, counted: not an engine-backed callable for the sampler, so it is stepped from the host
        def __call__(self, x, t, **k):
            calls.append(1)
            return model.forward_with_cfg(x, t, **k)

    fn.solver.use_engine = False
    torch.manual_seed(77)
    want = fn(z, model.forward_with_cfg, **kw)
    torch.manual_seed(77)
    counted = fn(z, Counted(), **kw)
    # twice the engine's count; the Tweedie rule reads the score only and the Euler rule the drift only - ONE evaluation in the host loop too
    assert len(calls) == 2 * nfe - (last_step in ("Tweedie", "Euler")), (len(calls), nfe)
    assert len(got) == len(want) == n
    for i, (a, b, c) in enumerate(zip(got, want, counted)):
        assert a.dtype == b.dtype and a.shape == b.shape, (i, a.dtype, b.dtype)
        assert torch.isfinite(b.float()).all(), i
        assert torch.equal(b, c), i
        assert torch.equal(a, b), (i, rel_l2(a, b))
    # solver.sample alone: the loop without the last step, the engine path again
    fn.solver.use_engine = True
    torch.manual_seed(77)
    loop = fn.solver.sample(z, model.forward_with_cfg, **kw)
    assert len(loop) == n - 1 and all(torch.equal(a, b) for a, b in zip(loop, want)) and model._engine.last_nfe() == (n - 1) * stages


def test_the_callable_protocol_is_unchanged_for_other_callables_and_predictions(golden_dir):
    """a wrapped callable, score prediction and the "constant" form run the host loop exactly as before (2 evaluations per stage through
    the callable; "constant" fails in the reference's own th.sqrt)"""
    model, z, kw = _model(golden_dir, "imagenet")
    z = z.to("cuda", torch.bfloat16)
    calls = []

    def wrapped(x, t, **k):
        calls.append(1)
        return model.forward_with_cfg(x, t, **k)

    torch.manual_seed(5)
    xs = Sampler(create_transport("Linear", "score", None, None, None)).sample_sde(diffusion_form="sigma", num_steps=4)(z, model.forward_with_cfg, **kw)
    assert len(xs) == 4
    before = model._engine.last_nfe()
    torch.manual_seed(5)
    xs2 = Sampler(create_transport("Linear", "score", None, None, None)).sample_sde(diffusion_form="sigma", num_steps=4)(z, wrapped, **kw)
    assert len(calls) == 8 and all(torch.equal(a, b) for a, b in zip(xs, xs2)) and model._engine.last_nfe() == before
    with pytest.raises(TypeError):
        Sampler(create_transport("Linear", "velocity", None, None, None)).sample_sde(diffusion_form="constant", num_steps=4)(z, model.forward_with_cfg, **kw)


# ---- reference-held ------------------------------------------------------------------------------------------------------------------
def test_engine_trajectory_vs_the_unmodified_reference_sampler(golden_dir):
    """bf16 state, the fixture's draws (same seed): rel_l2(engine, ref fp32) <= 1.5 x min(rel_l2 of the stored bf16 realisations) at every
    stored step"""
    g = np.load(os.path.join(golden_dir, "sde_imagenet_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    m = models.imagenet.DiT_Llama(**cfg.ctor_kwargs())
    m.load_state_dict(synth.synth_state_dict(cfg, seed=int(g["seed_w"])), strict=True)
    m = m.eval().to("cuda", torch.bfloat16)
    z, y = torch.from_numpy(g["z"]).to("cuda", torch.bfloat16), torch.from_numpy(g["y"]).cuda()
    cases, paths = json.loads(str(g["cases"])), json.loads(str(g["paths"]))
    n = int(g["num_steps"])
    for name, kw in cases.items():
        fn = Sampler(create_transport(paths[name], "velocity", None, None, None)).sample_sde(num_steps=n, **kw)
        torch.manual_seed(int(g["seed"]))
        got = fn(z, m.forward_with_cfg, y=y, cfg_scale=float(g["cfg_scale"]))
        assert len(got) == n and got[-1].dtype == torch.float32 and all(x.dtype == torch.bfloat16 for x in got[:-1])
        ref = list(torch.from_numpy(g[f"{name}_ref"])) + [torch.from_numpy(g[f"{name}_ref_last"])]
        real = []
        for key in ("refbf16", "refbf16ac"):
            loop = torch.from_numpy(g[f"{name}_{key}"]).view(torch.bfloat16).float()
            real.append(list(loop) + [torch.from_numpy(g[f"{name}_{key}_last"])])
        for i in range(n):
            floor = min(rel_l2(r[i], ref[i]) for r in real)
            err = rel_l2(got[i], ref[i])
            print(f"{name} step {i}: engine vs ref fp32 {err:.3e}   floor (reference's own bf16) {floor:.3e}   gate {1.5 * floor:.3e}")
        for i in range(n):
            floor = min(rel_l2(r[i], ref[i]) for r in real)
            assert rel_l2(got[i], ref[i]) <= 1.5 * floor, (name, i, rel_l2(got[i], ref[i]), floor)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(golden_dir):
    model, z, kw = _model(golden_dir, "imagenet")
    z = z.to("cuda", torch.bfloat16)
    model.forward_with_cfg(z, torch.full((z.shape[0],), 0.5, device="cuda"), **kw)  # engine + labels
    eng = model._engine
    L = lib()
    n = 4
    steps, last = I.sde_table(path.ICPlan(), "sigma", 1.0, torch.linspace(0, 0.96, n), torch.tensor(0.32), "Heun", z, "Mean", 0.04, 0.96)
    noise = torch.randn((n - 1,) + tuple(z.shape), device="cuda").to(torch.bfloat16)
    traj, fin = torch.empty_like(noise), torch.empty_like(z, dtype=torch.float32)
    a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)

    def call(steps_t, n_steps, method, last_step, last_t):
        sp = C.cast(steps_t.contiguous().data_ptr(), C.POINTER(C.c_float))
        lp = C.cast(last_t.contiguous().data_ptr(), C.POINTER(C.c_float))
        return L.lt_sample_sde(eng.handle, P(z), P(noise), P(traj), P(fin), sp, n_steps, method, last_step, lp, 1, C.byref(a), stream()), L.lt_last_error()

    rc, msg = call(steps, n, 7, _lib.LT_SDE_LAST_MEAN, last)
    assert rc != 0 and b"unknown method" in msg
    rc, msg = call(steps, n, _lib.LT_SDE_HEUN, 9, last)
    assert rc != 0 and b"unknown last_step" in msg
    rc, msg = call(steps, 1, _lib.LT_SDE_HEUN, _lib.LT_SDE_LAST_MEAN, last)
    assert rc != 0 and b"n_steps" in msg
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        s2 = steps.clone()
        s2[3, 2] = bad
        rc, msg = call(s2, n, _lib.LT_SDE_HEUN, _lib.LT_SDE_LAST_MEAN, last)
        assert rc != 0 and b"var" in msg and b"not finite and positive" in msg, (bad, msg)
        l2 = last.clone()
        l2[2] = bad
        rc, msg = call(steps, n, _lib.LT_SDE_HEUN, _lib.LT_SDE_LAST_TWEEDIE, l2)
        assert rc != 0 and b"var" in msg and b"last step" in msg, (bad, msg)
    rc, msg = call(steps, n, _lib.LT_SDE_HEUN, _lib.LT_SDE_LAST_MEAN, last)  # and the same arguments untouched are served
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert eng.last_nfe() == (n - 1) * 2 + 1 and torch.isfinite(fin).all()
    with pytest.raises(_lib.LuminaLibError, match="not in"):
        eng.sample_sde(z, noise, steps, last, "Milstein", "Mean", use_cfg=True, cfg_scale=4.0)
