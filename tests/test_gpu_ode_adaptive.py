"""-m gpu: adaptive Runge-Kutta sampling inside the engine (lt_sample_ode_adaptive, csrc/ode_adaptive.hip).

* the fused kernels (lt_op_rk_stage / _error_norm / _dense / _interp) against the host loop's own tensor expressions
  (transport/integrators.py: adaptive_odeint) run by torch on the same device: every output word equal, at bf16 and fp32, with a tail, in the
  unaligned one-element form and over more than one workgroup; the operand rules those expressions rest on asserted on their own;
* the norm against float64: with x = sqrt(mean(q^2)) in float64 the kernel returns float32(x); the other fp32 neighbour passes only where x
  lies within 2^-30 (relative) of the midpoint between the two - float64 accumulation of <= 2^19 exact terms errs below 2^-33, a margin of
  8 - and two runs return the same word;
* whole trajectories: the one-call path against ``adaptive_odeint`` driven by the same bound method, with the engine's norm
  (lt_op_rms_norm) as ``norm=`` and the engine's first step as ``first_step=``: every state, every count and every dt equal;
* the default path (first_step from the engine's own heuristic) against the oracle-driven solver under the gates of
  test_gpu_samplers.test_dopri5_on_the_engine_vs_oracle_driven_solver;
* the routing of ``ode.sample`` and the refusals by name."""
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
from oracle import synth
from oracle import variants_oracle as V

from gpu_util import P, lib, rel_l2, stream

pytestmark = pytest.mark.gpu

DT = 0.0371  # not a bf16 value: dty = bf16(dt) differs from dt
SHAPES = [(105, 0), (2048, 0), (2048, 1), (105, 1), (8 * 256 * 3 + 5, 0)]  # (n, offset in elements): tail, whole groups, unaligned, several workgroups


def _code(dtype):
    return _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32


def _rand(n, off, dtype, gen, scale=1.0):
    t = (torch.randn(n + off, generator=gen, device="cuda") * scale).to(dtype)[off:]
    assert t.data_ptr() % 16 == (0 if off == 0 else t.element_size() * off)
    return t


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _floats(vs):
    return (C.c_float * len(vs))(*[float(v) for v in vs])


def _nan_like(t, off):
    return torch.full((t.numel() + off,), float("nan"), dtype=t.dtype, device=t.device)[off:]


WS = None


def _ws():
    global WS
    if WS is None:
        WS = torch.empty(_lib.LT_RK_WS_BYTES // 8, dtype=torch.float64, device="cuda")
    return WS


# ---- the host loop's expressions, as integrators.py writes them --------------------------------------------------------------------
def chain(k, coef):
    acc = k[0] * coef[0]
    for kj, cj in zip(k[1:], coef[1:]):
        if cj != 0.0:
            acc = acc + kj * cj
    return acc


def stage(y, dty, k, coef):
    return y + dty * chain(k, coef)


def err_q(y, y1, dty, k, c_err, rtol, atol):
    err = dty * chain(k, c_err)
    tol = atol + rtol * torch.max(y.abs(), y1.abs())
    return err / tol


def dense(y, y1, y_mid, fy, f_1, dty):
    a = 2 * dty * (f_1 - fy) - 8 * (y1 + y) + 16 * y_mid
    b = dty * (5 * fy - 3 * f_1) + 18 * y + 14 * y1 - 32 * y_mid
    c = dty * (f_1 - 4 * fy) - 11 * y - 5 * y1 + 16 * y_mid
    return [y, dty * fy, c, b, a]


def interp(coeffs, x):
    total = coeffs[0] + x * coeffs[1]
    xp = x
    for cf in coeffs[2:]:
        xp = xp * x
        total = total + xp * cf
    return total


def op_stage(y, k, coef, dt, off):
    out = _nan_like(y, off)
    _lib.check(lib().lt_op_rk_stage(P(y), _ptrs(k), _floats(coef), len(k), dt, P(out), y.numel(), _code(y.dtype), stream()), "lt_op_rk_stage")
    return out


def op_rms(x, sub=None, y0=None, rtol=0.0, atol=0.0, q=None):
    out = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib().lt_op_rms_norm(P(x), P(sub), P(y0), rtol, atol, P(q), P(_ws()), P(out), x.numel(), _code(x.dtype), stream()), "lt_op_rms_norm")
    return out[0]


# ---- operand rules -----------------------------------------------------------------------------------------------------------------
def test_operand_rules_of_the_host_loops_expressions():
    """what the kernels' rounding points rest on, asserted of torch itself on this device"""
    g = torch.Generator(device="cuda").manual_seed(3)
    k = _rand(4096, 0, torch.bfloat16, g)
    beta = 9017 / 3168
    # a Python float times a bf16 tensor: ONE rounding of the fp32 product with the fp32 of the double - not a product with bf16(beta)
    assert torch.equal(k * beta, (k.float() * float(np.float32(beta))).to(torch.bfloat16))
    assert not torch.equal(k * beta, k * torch.tensor(beta, device="cuda").to(torch.bfloat16))
    # the 0-dim DEVICE tensor dty = dt.to(bf16): the product sees bf16(dt)
    dt = torch.tensor(DT, device="cuda")
    dty = dt.to(torch.bfloat16)
    assert dty.dtype == torch.bfloat16 and (dty * k).dtype == torch.bfloat16
    assert torch.equal(dty * k, (dty.float() * k.float()).to(torch.bfloat16))
    assert not torch.equal(dty * k, (dt * k.float()).to(torch.bfloat16))
    # an integer factor is an fp32 scalar: one rounding; 2 * dty stays a 0-dim bf16 tensor
    for f in (3, 5, 11, 14, 18):
        assert torch.equal(f * k, (k.float() * float(f)).to(torch.bfloat16))
    assert (2 * dty).dtype == torch.bfloat16 and (2 * dty).dim() == 0
    # x and its powers in the interpolation are 0-dim tensors of the state dtype: xp * x rounds every time
    x = torch.tensor(0.3, device="cuda").to(torch.bfloat16)
    assert (x * x).dtype == torch.bfloat16 and float(x * x) == float((x.float() * x.float()).to(torch.bfloat16))
    # atol + rtol * tensor: fp32 scalars, a rounding after each
    m = k.abs()
    assert torch.equal(2e-2 + 2e-2 * m, ((m.float() * float(np.float32(2e-2))).to(torch.bfloat16).float() + float(np.float32(2e-2))).to(torch.bfloat16))


# ---- kernels, word for word ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("method", I.ADAPTIVE_METHODS)
def test_kernels_equal_the_torch_expressions_word_for_word(method, dtype):
    ALPHA, BETA, C_SOL, C_ERR, C_MID, _ = I._TABLEAUS[method]
    g = torch.Generator(device="cuda").manual_seed(17)
    dty = torch.tensor(DT, device="cuda").to(dtype)
    rtol, atol = 2e-2, 1e-2
    for n, off in SHAPES:
        tag = (method, dtype, n, off)
        y = _rand(n, off, dtype, g)
        k = [_rand(n, off, dtype, g, 1.5) for _ in range(len(C_SOL))]
        # every stage, then the solution and mid-point chains (the same kernel)
        for i, beta in enumerate(BETA):
            assert torch.equal(op_stage(y, k[:i + 1], beta, DT, off), stage(y, dty, k[:i + 1], beta)), ("stage", i) + tag
        y1 = stage(y, dty, k, C_SOL)
        assert torch.equal(op_stage(y, k, C_SOL, DT, off), y1), ("c_sol",) + tag
        y_mid = stage(y, dty, k, C_MID)
        assert torch.equal(op_stage(y, k, C_MID, DT, off), y_mid), ("c_mid",) + tag
        # error / tolerance / quotient, and the norm of the quotient
        want_q = err_q(y, y1, dty, k, C_ERR, rtol, atol)
        q = _nan_like(y, off)
        nrm = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib().lt_op_rk_error_norm(P(y), P(y1), _ptrs(k), _floats(C_ERR), len(k), DT, rtol, atol, P(q), P(_ws()), P(nrm), n, _code(dtype),
                                             stream()), "lt_op_rk_error_norm")
        assert want_q.dtype == dtype and torch.equal(q, want_q), ("err",) + tag
        assert float(nrm[0]) == float(op_rms(q)), ("err norm == rms of its quotient",) + tag
        _check_norm(float(nrm[0]), want_q, tag)
        # dense output and interpolation
        want = dense(y, y1, y_mid, k[0], k[-1], dty)
        got = [_nan_like(y, off) for _ in range(4)]
        _lib.check(lib().lt_op_rk_dense(P(y), P(y1), P(y_mid), P(k[0]), P(k[-1]), DT, P(got[0]), P(got[1]), P(got[2]), P(got[3]), n, _code(dtype),
                                        stream()), "lt_op_rk_dense")
        for j, name in enumerate(("c1", "c", "b", "a")):
            assert want[j + 1].dtype == dtype and torch.equal(got[j], want[j + 1]), (name,) + tag
        for xv in (0.3, 0.8125, 1.0):
            x = torch.tensor(xv, device="cuda").to(dtype)
            out = _nan_like(y, off)
            _lib.check(lib().lt_op_rk_interp(_ptrs([y] + got), xv, P(out), n, _code(dtype), stream()), "lt_op_rk_interp")
            assert torch.equal(out, interp(want, x)), ("interp", xv) + tag
        # the initial-step heuristic: y0 + h0 f0 and the three scaled norms
        assert torch.equal(op_stage(y, k[:1], [1.0], DT, off), y + dty * k[0]), ("y0 + h0 f0",) + tag
        scale = atol + y.abs() * rtol
        for x_, sub_, want_q in ((y, None, y / scale), (k[0], None, k[0] / scale), (k[1], k[0], (k[1] - k[0]) / scale)):
            q = _nan_like(y, off)
            got_n = float(op_rms(x_, sub_, y, rtol, atol, q))
            assert torch.equal(q, want_q), ("scaled", sub_ is not None) + tag
            _check_norm(got_n, want_q, tag)


def _check_norm(got, q, tag):
    x = float(q.double().pow(2).mean().sqrt())
    r = np.float32(x)
    if np.float32(got) == r:
        return
    nb = np.nextafter(r, np.float32(np.inf) if got > float(r) else np.float32(-np.inf))
    mid = (float(r) + float(nb)) / 2
    assert np.float32(got) == nb and abs(x - mid) <= 2.0 ** -30 * x, ("norm", got, x, float(r)) + tuple(tag)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [105, 2048, 524288])  # the last: 8 x 4 x 128 x 128, the engine's largest state; the multi-workgroup tree
def test_norm_is_the_fp32_of_the_float64_value_and_the_same_on_every_run(n, dtype):
    g = torch.Generator(device="cuda").manual_seed(n)
    for off in (0, 1):
        q = _rand(n, off, dtype, g, 0.7)
        a = op_rms(q).clone()
        b = op_rms(q).clone()
        assert a.view(torch.int32).item() == b.view(torch.int32).item()
        _check_norm(float(a), q, (n, dtype, off))
    # a norm that float32 accumulation gets wrong: 2^19 terms of very different size
    q = torch.cat([torch.full((1,), 4096.0, device="cuda"), torch.full((n - 1,), 2.0 ** -7, device="cuda")]).to(dtype)
    _check_norm(float(op_rms(q)), q, (n, dtype, "spread"))


# ---- whole trajectories --------------------------------------------------------------------------------------------------------------
def _imagenet(golden_dir):
    g = np.load(os.path.join(golden_dir, "imagenet_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    m = models.imagenet.DiT_Llama(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=True)
    m = m.eval().to("cuda", torch.bfloat16)
    return g, cfg, sd, m, torch.from_numpy(g["z"]), dict(y=torch.from_numpy(g["y"]).cuda(), cfg_scale=4.0)


def _next(golden_dir):
    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    m = models.NextDiT(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=True)
    m = m.eval().to("cuda", torch.bfloat16)
    kw = dict(cap_feats=torch.from_numpy(g["cap"]).to("cuda", torch.bfloat16), cap_mask=torch.from_numpy(g["mask"]).cuda(), cfg_scale=4.0,
              proportional_attn=True, base_seqlen=16)
    return g, cfg, sd, m, torch.from_numpy(g["z"]), kw


_MODELS = {}


def _model(golden_dir, family):
    if family not in _MODELS:
        _MODELS[family] = (_imagenet if family == "imagenet" else _next)(golden_dir)
    return _MODELS[family]


def _solver(method, rtol, atol, num_steps=4):
    fn = Sampler(create_transport("Linear", "velocity", None, None, None)).sample_ode(sampling_method=method, num_steps=num_steps, atol=atol,
                                                                                       rtol=rtol)
    return fn, fn.__self__


def _both_paths(golden_dir, family, method, dtype, rtol, atol, first_step):
    _, _, _, model, z, kw = _model(golden_dir, family)
    x = z.to("cuda", dtype)
    fn, solver = _solver(method, rtol, atol)
    solver.first_step = first_step
    got = fn(x, model.forward_with_cfg, **kw)
    st = solver.stats
    # the host loop through the same bound method, measuring with the engine's norm and starting with the engine's first step
    hs = {}
    B = x.shape[0]
    want = I.adaptive_odeint(lambda t, y: model.forward_with_cfg(y, torch.ones(B, device="cuda") * t, **kw), x, solver.t.cuda(), method=method,
                             rtol=rtol, atol=atol, norm=lambda v: op_rms(v.contiguous()), first_step=st["first_step"], stats=hs)
    return got, st, want, hs


CASES = [("imagenet", "dopri5", torch.bfloat16), ("imagenet", "dopri5", torch.float32), ("next", "dopri5", torch.bfloat16),
         ("next", "dopri5", torch.float32), ("imagenet", "bosh3", torch.bfloat16), ("next", "fehlberg2", torch.float32),
         ("imagenet", "adaptive_heun", torch.bfloat16)]


@pytest.mark.parametrize("family,method,dtype", CASES)
def test_one_call_trajectory_equals_the_host_loop_bit_for_bit(golden_dir, family, method, dtype):
    got, st, want, hs = _both_paths(golden_dir, family, method, dtype, 2e-2, 2e-2, None)
    print(f"{family} {method} {dtype}: nfe {st['nfe']} accepted {st['accepted']} rejected {st['rejected']} first_step {st['first_step']:.6g}")
    S = len(I._TABLEAUS[method][0])
    assert got.shape == want.shape == (4,) + tuple(got.shape[1:]) and got.dtype == dtype
    assert st["nfe"] == 2 + S * (st["accepted"] + st["rejected"]) and st["accepted"] >= 1
    # the host loop was handed the first step: it makes one evaluation less in front of the first step
    assert (hs["nfe"] + 1, hs["accepted"], hs["rejected"]) == (st["nfe"], st["accepted"], st["rejected"])
    assert hs["dt"] == st["dt"] and len(st["dt"]) == st["accepted"] + st["rejected"]
    for i in range(4):
        assert torch.equal(got[i], want[i]), (i, rel_l2(got[i], want[i]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_first_step_of_the_whole_interval(golden_dir, dtype):
    """first_step = t1 - t0: used as given (one evaluation in front of the first step); whether the controller rejects it is the model's
    business (the reject branch is held by tests/test_ode_adaptive_cpu.py) - the counts are printed"""
    got, st, want, hs = _both_paths(golden_dir, "imagenet", "dopri5", dtype, 2e-2, 2e-2, 1.0)
    print(f"first_step 1.0 {dtype}: nfe {st['nfe']} accepted {st['accepted']} rejected {st['rejected']} dt {st['dt']}")
    assert st["first_step"] == 1.0 and st["dt"][0] == 1.0
    assert st["nfe"] == 1 + 6 * (st["accepted"] + st["rejected"])
    assert (hs["nfe"], hs["accepted"], hs["rejected"], hs["dt"]) == (st["nfe"], st["accepted"], st["rejected"], st["dt"])
    assert torch.equal(got, want)


@pytest.mark.parametrize("state_dtype", [torch.float32, torch.bfloat16])
def test_default_path_vs_oracle_driven_solver(golden_dir, state_dtype):
    """the construction and gates of test_gpu_samplers.test_dopri5_on_the_engine_vs_oracle_driven_solver, with the bound method: one call"""
    g, cfg, sd, model, z, kw = _model(golden_dir, "imagenet")
    tr = create_transport("Linear", "velocity", None, None, None)
    skw = dict(sampling_method="dopri5", num_steps=4, atol=2e-2, rtol=2e-2)
    fn = Sampler(tr).sample_ode(**skw)
    got = fn(z.to("cuda", state_dtype), model.forward_with_cfg, **kw)
    st = fn.__self__.stats
    nfe = model._engine.last_nfe()
    ref = Sampler(tr).sample_ode(**skw)(z.to(state_dtype), lambda x, t, **k: V.imagenet_forward_with_cfg(sd, cfg, x.float(), t, **k).to(state_dtype),
                                        y=kw["y"].cpu(), cfg_scale=4.0)
    assert got.shape == ref.shape == (4,) + tuple(z.shape) and got.dtype == state_dtype
    assert nfe >= 8 and nfe == st["nfe"] == 2 + 6 * (st["accepted"] + st["rejected"])
    assert torch.equal(got[0].float().cpu(), z.to(state_dtype).float())
    tol = 6e-2 if state_dtype == torch.float32 else 1e-1
    for i in (1, 2, 3):
        print(f"{state_dtype} grid point {i}: rel-L2 {rel_l2(got[i], ref[i]):.3e}")
    for i in (1, 2, 3):
        assert rel_l2(got[i], ref[i]) < tol, (i, rel_l2(got[i], ref[i]))


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
def test_routing_of_ode_sample(golden_dir, monkeypatch):
    _, _, _, model, z, kw = _model(golden_dir, "imagenet")
    calls = []
    real = type(model)._engine_sample_ode_adaptive

    def counted(self, *a, **k):
        calls.append(a[2])
        return real(self, *a, **k)

    monkeypatch.setattr(type(model), "_engine_sample_ode_adaptive", counted)
    x = z.to("cuda", torch.bfloat16)
    fn, solver = _solver("dopri5", 2e-2, 2e-2)
    one_call = fn(x, model.forward_with_cfg, **kw)
    assert calls == ["dopri5"] and solver.stats["nfe"] == model._engine.last_nfe()
    # switched off: the host loop through the same bound method
    solver.use_engine = False
    host = fn(x, model.forward_with_cfg, **kw)
    assert calls == ["dopri5"] and host.shape == one_call.shape
    assert rel_l2(host, one_call) < 5e-2  # the same solver on the same model; the step sequences may drift by the norm's low bits
    # a wrapped callable
    fn, solver = _solver("dopri5", 2e-2, 2e-2)
    fn(x, lambda xx, t, **k: model.forward_with_cfg(xx, t, **k), **kw)
    assert calls == ["dopri5"]
    # a tuple state (the likelihood ODE's shape of state): the host loop, whatever the callable
    tup = I.ode(drift=lambda st, t, m, **k: (m(st[0], t, **k), torch.zeros_like(st[1])), t0=0.0, t1=1.0, sampler_type="dopri5", num_steps=2, atol=2e-2,
                rtol=2e-2)
    tup.drift.is_plain_velocity = True
    out = tup.sample((x, torch.zeros(x.shape[0], device="cuda")), model.forward_with_cfg, **kw)
    assert isinstance(out, tuple) and calls == ["dopri5"]
    # a CPU state never reaches the engine path: the model refuses it by name from inside the host loop
    fn, solver = _solver("dopri5", 2e-2, 2e-2)
    with pytest.raises(_lib.LuminaLibError):
        fn(z.to(torch.bfloat16), model.forward_with_cfg, y=kw["y"].cpu(), cfg_scale=4.0)
    assert calls == ["dopri5"]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(golden_dir):
    _, _, _, model, z, kw = _model(golden_dir, "imagenet")
    x = z.to("cuda", torch.bfloat16)
    eng, args = model._engine_sampler_args(x, True, dict(kw))
    grid = torch.linspace(0.0, 1.0, 4)

    def run(grid=grid, method="dopri5", rtol=2e-2, atol=2e-2, **k):
        return eng.sample_ode_adaptive(x, grid, method, use_cfg=True, rtol=rtol, atol=atol, **k, **args)

    with pytest.raises(_lib.LuminaLibError, match="adaptive method 'rk4'"):
        run(method="rk4")
    a = eng._step_args(x, 4.0, 1.0, 1.0, None, False)
    garr = (C.c_float * 4)(0.0, 0.25, 0.5, 1.0)
    out = torch.empty((4,) + tuple(x.shape), dtype=x.dtype, device="cuda")
    for method in (_lib.LT_ODE_RK4, 7, -1):
        rc = lib().lt_sample_ode_adaptive(eng.handle, P(x), P(out), garr, 4, method, 2e-2, 2e-2, 0.0, 100, 1, 1, C.byref(a), stream(), None)
        assert rc != 0 and b"unknown method" in lib().lt_last_error()
    with pytest.raises(_lib.LuminaLibError, match="max_steps 1 exceeded"):
        run(rtol=1e-7, atol=1e-7, max_steps=1)
    with pytest.raises(_lib.LuminaLibError, match="rtol 0 and atol"):
        run(rtol=0.0)
    with pytest.raises(_lib.LuminaLibError, match="must be finite and positive"):
        run(atol=float("nan"))
    with pytest.raises(_lib.LuminaLibError, match="at least 2 grid points"):
        run(grid=torch.tensor([0.0]))
    with pytest.raises(_lib.LuminaLibError, match="not strictly increasing"):
        run(grid=torch.tensor([0.0, 0.6, 0.5, 1.0]))
    with pytest.raises(_lib.LuminaLibError, match="not strictly increasing"):
        run(grid=torch.tensor([1.0, 0.0]))
    # the engine is whole after the refusals
    got, st = run()
    assert st["accepted"] >= 1 and bool(torch.isfinite(got.float()).all())
