"""GPU: linear multistep ODE sampling - lt_op_ode_multistep, lt_sample_ode_multistep, lt_sample_ode_multistep_packed.  Everything but
one named figure is exact: no tolerance.

* kernel: every output word of a step equals the float64 restatement of the rounding chain (tests/exact_multistep.py) - the tail alone, one
  vector, one vector and an element, several blocks and a tail; bf16 and fp32; 1 .. 4 slopes; with and without the corrector; bf16 products on
  midpoints and an fp32 case a fused multiply-add would change; the aligned and the scalar path agree; guard words stay;
* loop: each method's trajectory in ONE call equals the host loop ``transport.multistep.multistep_odeint`` around the same model at every slot,
  with N evaluations;
* a guidance table with a conditional-only evaluation under a rescale / norm-limit rule equals the host loop, and a second table replays the
  same two captured graphs;
* a packed batch; the transport front ends and the ``sample.py`` driver; refusals by name."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport import multistep as MS
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

import exact_multistep as X
from gpu_util import P, lib, rel_l2, stream
from test_gpu_model import TOL_CFG4  # the gate of the packed forward_with_cfg tests (tests/test_gpu_packed_cfg.py): imported, not restated
from test_gpu_sde import _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
METHODS = MS.MULTISTEP_METHODS
N_INT = 5  # more than 4 intervals: the slope ring wraps, and ab3 / abm3 run at full order
_CACHE = {}
GUARD = 32  # words in front of and behind every output: 64 / 128 bytes, so the buffer behind the guard is 16-byte aligned


# ---- kernel --------------------------------------------------------------------------------------------------------------------------
def _weights(ns, fma):
    if fma:
        return [0.0] * 4, [X.FMA_WEIGHT, 0.0, 0.0, 0.0]
    w = list(X.MIDPOINT_WEIGHTS)
    return w[:ns] + [0.0] * (4 - ns), w[::-1][4 - ns:] + [0.0] * (4 - ns)


def _run_op(dtype, n, y_prev, ks, ns, a, b, has_corr, shift):
    """the op on device copies that start ``shift`` words behind a 16-byte boundary; returns (y, p) and whether every guard word survived"""
    code = _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32

    def place(v):
        buf = torch.zeros(GUARD + shift + n + GUARD, dtype=dtype, device="cuda")
        buf[GUARD + shift:GUARD + shift + n] = v.cuda()
        return buf

    ins = [place(v) for v in [y_prev] + list(ks[:ns])]
    outs = [torch.full((GUARD + shift + n + GUARD,), 1.5, dtype=dtype, device="cuda") for _ in range(2)]
    at = lambda t: C.c_void_p(t.data_ptr() + (GUARD + shift) * t.element_size())  # noqa: E731
    karr = (C.c_void_p * 4)(*[at(t).value for t in ins[1:]] + [0] * (4 - ns))
    F4 = C.c_float * 4
    rc = lib().lt_op_ode_multistep(at(ins[0]), karr, ns, F4(*a), F4(*b), has_corr, at(outs[0]), at(outs[1]), n, code, stream())
    assert rc == 0, lib().lt_last_error()
    torch.cuda.synchronize()
    lo, hi = GUARD + shift, GUARD + shift + n
    guards_ok = all(bool((o[:lo] == 1.5).all()) and bool((o[hi:] == 1.5).all()) for o in outs)
    return outs[0][lo:hi].cpu(), outs[1][lo:hi].cpu(), guards_ok


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2055])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_kernel_equals_the_chain_word_for_word(dtype, n):
    y_prev, *ks = X.operands(n, dtype, 11 + n)
    cases = [(ns, has_corr, False) for ns in (1, 2, 3, 4) for has_corr in (0, 1)] + [(1, 0, True)]
    for ns, has_corr, fma in cases:
        a, b = _weights(ns, fma)
        tag = (dtype, n, ns, has_corr, fma)
        wy, wp = X.chain64(y_prev, ks, a, b, has_corr, dtype)
        y, p, guards_ok = _run_op(dtype, n, y_prev, ks, ns, a, b, has_corr, 0)
        assert guards_ok, tag
        assert torch.equal(X.bits(p), X.bits(wp)), tag + (int((X.bits(p) != X.bits(wp)).sum()),)
        if has_corr:
            assert torch.equal(X.bits(y), X.bits(wy)), tag + (int((X.bits(y) != X.bits(wy)).sum()),)
        else:
            assert bool((y == 1.5).all()), tag  # one output: y_out is not written
        if fma and dtype == torch.float32 and n > 1:
            assert bool((p[1::4] == 0).all()), tag  # (a fused multiply-add gives 2^-24 here)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_scalar_path_agrees_with_the_vector_path(dtype):
    n = 2055
    y_prev, *ks = X.operands(n, dtype, 3)
    a, b = _weights(4, False)
    y0, p0, ok0 = _run_op(dtype, n, y_prev, ks, 4, a, b, 1, 0)
    y1, p1, ok1 = _run_op(dtype, n, y_prev, ks, 4, a, b, 1, 1)  # every pointer one word off a 16-byte boundary
    assert ok0 and ok1
    assert torch.equal(X.bits(y0), X.bits(y1)) and torch.equal(X.bits(p0), X.bits(p1))
    wy, wp = X.chain64(y_prev, ks, a, b, 1, dtype)
    assert torch.equal(X.bits(y1), X.bits(wy)) and torch.equal(X.bits(p1), X.bits(wp))


# ---- loop ----------------------------------------------------------------------------------------------------------------------------
def _next(golden_dir):
    if "next" not in _CACHE:
        model, z, kw = _model(golden_dir, "next")
        _CACHE["next"] = (model, kw)
    return _CACHE["next"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", METHODS)
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, kw = _next(golden_dir)
    o = ODE(N_INT + 1, method, 4)
    assert len(o.t) == N_INT + 1 and float(o.t[1] - o.t[0]) != float(o.t[2] - o.t[1])  # time-shifted: the variable-step weights matter
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(6)).to("cuda", dtype).repeat(2, 1, 1, 1)
    got = o.sample(z, model.forward_with_cfg, **kw)  # ONE lt_sample_ode_multistep call
    assert model._engine.last_nfe() == N_INT and model._engine.last_eval_rows() == 2 * N_INT
    calls = []

    def f(tt, y):
        calls.append(1)
        return model.forward_with_cfg(y, torch.ones(2, device="cuda") * tt, **kw)

    want = MS.multistep_odeint(f, z, o.t.cuda(), method)
    assert len(calls) == N_INT
    assert got.shape == want.shape == (N_INT + 1,) + tuple(z.shape) and got.dtype == dtype
    assert bool(torch.isfinite(want.float()).all())
    for i in range(N_INT + 1):
        assert torch.equal(got[i], want[i]), (method, dtype, i, int((got[i] != want[i]).sum()))
    assert not torch.equal(got[-1], ODE(N_INT + 1, "euler", 4).sample(z, model.forward_with_cfg, **kw)[-1])
    final = model._engine.sample_ode_multistep(z, o.t, method, use_cfg=True, cfg_scale=4.0, proportional_attn=True, base_seqlen=16,
                                               return_trajectory=False)
    assert torch.equal(final, got[-1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_a_callers_table_with_rows_without_a_corrector_equals_the_host_loop(golden_dir, dtype):
    """the table is the contract: abm3's, with the corrector halves of rows 2 and 4 (behind the ring's wrap) zeroed - there y_i = p_i, which the
    engine has in another buffer than y_{i-1} - and row 3 correcting from that y_2.  Every slot of a record pre-filled with NaN is held to
    ``multistep_odeint(table=)``."""
    model, kw = _next(golden_dir)
    tgrid = ODE(N_INT + 1, "abm3", 4).t
    tab = MS.multistep_table(tgrid, "abm3")
    tab[2, :4] = 0
    tab[4, :4] = 0
    assert [MS.used(r[:4].tolist()) for r in tab] == [0, 2, 0, 4, 0]
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(12)).to("cuda", dtype).repeat(2, 1, 1, 1)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), **kw)  # engine, weights, prompt
    eng = model._engine

    def f(tt, y):
        return model.forward_with_cfg(y, torch.ones(2, device="cuda") * tt, **kw)

    want = MS.multistep_odeint(f, z, tgrid.cuda(), "abm3", table=tab)
    plain = MS.multistep_odeint(f, z, tgrid.cuda(), "abm3")
    assert not torch.equal(want[2], plain[2]) and not torch.equal(want[-1], plain[-1])  # the zeroed rows matter
    # through the C entry, into a record that holds NaN: every slot must be written
    n = z.numel()
    rec = torch.full((N_INT + 2, n), float("nan"), dtype=dtype, device="cuda")
    a = eng._step_args(z, 4.0, 1.0, 1.0, 16, True)
    grid = (C.c_float * (N_INT + 1))(*[float(v) for v in tgrid.tolist()])
    coef = (C.c_float * (N_INT * 8))(*tab.reshape(-1).tolist())
    rc = lib().lt_sample_ode_multistep(eng.handle, P(z), P(rec), P(rec[N_INT + 1]), grid, N_INT + 1, coef, 1, None, 0.0, float("inf"), 1, 1,
                                       C.byref(a), stream())
    assert rc == 0, lib().lt_last_error()
    torch.cuda.synchronize()
    assert eng.last_nfe() == N_INT
    for i in range(N_INT + 1):
        assert torch.equal(rec[i].view_as(z), want[i]), (dtype, i, int((rec[i].view_as(z) != want[i]).sum()))
    assert torch.equal(rec[N_INT + 1].view_as(z), want[-1])
    # ... and through the Python layer
    got = eng.sample_ode_multistep(z, tgrid, None, coef=tab, use_cfg=True, cfg_scale=4.0, proportional_attn=True, base_seqlen=16)
    assert torch.equal(got, want)
    with pytest.raises(_lib.LuminaLibError, match="coef must be"):
        eng.sample_ode_multistep(z, tgrid, None, coef=tab[:3], use_cfg=True)


def test_guidance_table_and_rule_equal_the_host_loop_and_replay_two_graphs(golden_dir):
    model, _, kw = _model(golden_dir, "next")  # a fresh engine: no key has been used
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    step_kw = dict(proportional_attn=True, base_seqlen=16)
    H, W = 50, 82  # 25 x 41 = 1025 tokens: the smallest latent whose B' = 1 evaluation has more than 1024 rows (the graph path)
    tgrid = ODE(N_INT + 1, "abm2", 4).t
    table = torch.tensor([3.0, 2.0, 1.0, 4.5, 5.0])
    z = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(8)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), cap, cmask, 4.0, **step_kw)  # engine, weights, prompt
    eng = model._engine
    before = eng.graph_replays()
    got = model.sample_ode_cfg_schedule(z, tgrid, table, cap, cmask, method="abm2", return_trajectory=True, rescale=0.7, norm_limit=0.9, **step_kw)
    B = 2
    assert eng.last_nfe() == N_INT and eng.last_eval_rows() == N_INT * B - B // 2
    assert eng.graph_replays() - before == (4 - 1) + (1 - 1)  # the first use of each of the two keys runs eagerly
    factors = []
    want = G.sample_cfg_multistep(model, z, tgrid, table, "abm2", rescale=0.7, norm_limit=0.9, factors=factors, cap_feats=cap, cap_mask=cmask, **step_kw)
    assert len(factors) == 4 and any(float(f) != 1.0 for f in factors)  # guided_rule ran per guided evaluation, and did something
    for i in range(N_INT + 1):
        assert torch.equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    # a second table: the same two captured graphs serve every evaluation
    table2 = torch.tensor([1.0, 2.5, 3.5, 1.0, 6.0])
    before = eng.graph_replays()
    got2 = model.sample_ode_cfg_schedule(z, tgrid, table2, cap, cmask, method="abm2", return_trajectory=True, rescale=0.7, norm_limit=0.9, **step_kw)
    assert eng.graph_replays() - before == N_INT and eng.last_eval_rows() == N_INT * B - 2 * (B // 2)
    want2 = G.sample_cfg_multistep(model, z, tgrid, table2, "abm2", rescale=0.7, norm_limit=0.9, cap_feats=cap, cap_mask=cmask, **step_kw)
    assert torch.equal(got2, want2) and not torch.equal(got2[-1], got[-1])
    # the table without the rule, through the transport front end
    o = ODE(N_INT + 1, "abm2", 4)
    via = o.sample(z, model.forward_with_cfg, cfg_table=table, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **step_kw)
    assert eng.last_nfe() == N_INT and eng.last_eval_rows() == N_INT * B - B // 2
    o.use_engine = False
    assert torch.equal(via, o.sample(z, model.forward_with_cfg, cfg_table=table, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **step_kw))
    # the Sampler front end (integrators.ode): the same table, then with the rule - one engine call each, the host loop with use_engine = False
    fn = Sampler(create_transport()).sample_ode(sampling_method="abm2", num_steps=N_INT + 1, time_shifting_factor=4.0)
    assert torch.equal(fn.__self__.t, tgrid)
    got3 = fn(z, model.forward_with_cfg, cfg_table=table, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **step_kw)
    assert eng.last_nfe() == N_INT and eng.last_eval_rows() == N_INT * B - B // 2 and torch.equal(got3, via)
    got4 = fn(z, model.forward_with_cfg, cfg_table=table, cfg_rescale=0.7, cfg_norm_limit=0.9, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **step_kw)
    assert eng.last_nfe() == N_INT and torch.equal(got4, got)
    fn.__self__.use_engine = False
    assert torch.equal(fn(z, model.forward_with_cfg, cfg_table=table, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **step_kw), via)


# ---- packed --------------------------------------------------------------------------------------------------------------------------
def test_packed_batch_of_two_sizes(golden_dir):
    """ab2 on two latents of different sizes.  The whole packed trajectory equals the host loop over forward_with_cfg_packed bit for bit.  Against
    the same call on one sample alone the condition is the one tests/test_gpu_packed_cfg.py holds packed batches to: the LONGEST sample equals
    its solo run bit for bit (its rows see no padding either way); the shorter one runs padded rows through other launches, and is held to
    TOL_CFG4, the gate that file imports for packed forward_with_cfg outputs."""
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(4)
    half = [torch.randn(4, 16, 16, generator=g).to("cuda", dtype), torch.randn(4, 8, 12, generator=g).to("cuda", dtype)]
    zs = half + [h.clone() for h in half]
    cf, cm = torch.cat([cap[:1], cap[:1], cap[1:], cap[1:]]), torch.cat([cmask[:1], cmask[:1], cmask[1:], cmask[1:]])
    tgrid = ODE(N_INT + 1, "ab2", 4).t
    got = model.sample_ode_packed(zs, tgrid, cf, cm, 4.0, method="ab2", return_trajectory=True)
    assert model._engine.last_nfe() == N_INT
    counts, shapes = [z.numel() for z in zs], [tuple(z.shape) for z in zs]

    def f(tt, flat):
        xs = [p.view(s) for p, s in zip(flat.split(counts), shapes)]
        tvec = torch.ones(len(zs), device="cuda") * tt
        return torch.cat([o.reshape(-1) for o in model.forward_with_cfg_packed(xs, tvec, cf, cm, 4.0)])

    slow = MS.multistep_odeint(f, torch.cat([z.reshape(-1) for z in zs]), tgrid.cuda(), "ab2")
    for b in range(4):
        want = torch.stack([slow[i].split(counts)[b].view(shapes[b]) for i in range(N_INT + 1)])
        assert torch.equal(got[b], want), b
    finals = model.sample_ode_packed(zs, tgrid, cf, cm, 4.0, method="ab2")
    for b in range(2):
        solo = model.sample_ode_packed([zs[b], zs[b]], tgrid, torch.cat([cf[b:b + 1], cf[b + 2:b + 3]]), torch.cat([cm[b:b + 1], cm[b + 2:b + 3]]),
                                       4.0, method="ab2")
        assert torch.equal(finals[b], got[b][-1])
        err = rel_l2(finals[b], solo[0])
        print(f"packed ab2 sample {b} {shapes[b]}: final state vs its solo run rel-L2 {err:.3e}")
        if b == 0:
            assert torch.equal(finals[b], solo[0]), err
        else:
            assert err < TOL_CFG4, err


# ---- front ends ----------------------------------------------------------------------------------------------------------------------
def test_front_ends_reach_the_engine_in_one_call(golden_dir, monkeypatch):
    model, kw = _next(golden_dir)
    calls = []
    inner = type(model)._engine_sample_ode_multistep

    def counted(self, x, tgrid, method, *a, **k):
        calls.append(method)
        return inner(self, x, tgrid, method, *a, **k)

    monkeypatch.setattr(type(model), "_engine_sample_ode_multistep", counted)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(2)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    fn = Sampler(create_transport()).sample_ode(sampling_method="abm3", num_steps=N_INT + 1, time_shifting_factor=4.0)
    got = fn(z, model.forward_with_cfg, **kw)
    assert calls == ["abm3"] and model._engine.last_nfe() == N_INT
    fn.__self__.use_engine = False
    want = fn(z, model.forward_with_cfg, **kw)
    assert calls == ["abm3"] and torch.equal(got, want) and got.shape == (N_INT + 1,) + tuple(z.shape)
    o = ODE(N_INT + 1, "abm3", 4.0)
    got2 = o.sample(z, model.forward_with_cfg, **kw)
    assert calls == ["abm3", "abm3"] and torch.equal(got2, got)
    o.use_engine = False
    assert torch.equal(o.sample(z, model.forward_with_cfg, **kw), got) and calls == ["abm3", "abm3"]
    # t_round_to_state_dtype = False reaches both paths: the model sees the unrounded fp32 time either way
    o.use_engine, o.t_round_to_state_dtype = True, False
    raw = o.sample(z, model.forward_with_cfg, **kw)
    assert calls == ["abm3"] * 3 and not torch.equal(raw[-1], got[-1])
    o.use_engine = False
    assert torch.equal(o.sample(z, model.forward_with_cfg, **kw), raw)
    calls.pop()
    # the plain forward of the cond row: the engine path without guidance
    o.use_engine, o.t_round_to_state_dtype = True, True
    plain = o.sample(z[:1], model.forward, cap_feats=kw["cap_feats"][:1].contiguous(), cap_mask=kw["cap_mask"][:1].contiguous())
    assert calls[-1] == "abm3" and len(calls) == 3 and model._engine.last_eval_rows() == N_INT and plain.shape == (N_INT + 1, 1, 4, 16, 16)


def test_sample_driver_with_a_multistep_solver_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_multistep_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_multistep_test"] = ctor
    (tmp_path / "prompts.txt").write_text("a red cube\n")
    gen = torch.Generator().manual_seed(3)
    table = {c: torch.randn(16, cfg.cap_feat_dim, generator=gen) for c in ("a red cube", "")}

    def encode(caps):
        feats = torch.stack([table[c] for c in caps]).to("cuda", torch.bfloat16)
        mask = torch.ones(len(caps), 16, dtype=torch.int64, device="cuda")
        mask[-1, 8:] = 0
        return feats, mask

    decoded = []

    def decode(lat):
        decoded.append(lat.clone())
        return torch.sigmoid(lat[:, :3].float())

    argv = ["--ckpt", str(ck), "--caption_path", str(tmp_path / "prompts.txt"), "--resolution", "256:128x128", "--num_sampling_steps", str(N_INT + 1),
            "--solver", "abm2", "--time_shifting_factor", "4", "--seed", "11", "--image_save_path", str(tmp_path / "out")]
    try:
        S.run(S.build_parser().parse_args(argv), encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
    finally:
        del models.__dict__["NextDiT_tiny_multistep_test"]
    model = built[0]
    assert (model._engine.last_nfe(), model._engine.last_eval_rows()) == (N_INT, 2 * N_INT)  # every evaluation lies in ONE call
    fn = Sampler(create_transport()).sample_ode(sampling_method="abm2", num_steps=N_INT + 1, time_shifting_factor=4.0)
    fn.__self__.use_engine = False  # the host loop
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    feats, mask = encode(["a red cube", ""])
    want = fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, proportional_attn=True, base_seqlen=256, scale_factor=1.0,
              scale_watershed=1.0)[-1][:1]
    assert len(decoded) == 1 and torch.equal(decoded[0], want / 0.13025)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    n = 2 * 4 * 16 * 16
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    t = torch.full((2,), 0.5, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0)  # engine, weights, a prompt of 2 rows
    eng, L = model._engine, lib()
    out = torch.full((8 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    grid = (C.c_float * 3)(0.0, 0.5, 1.0)
    F = C.c_float * 16
    good = F(*MS.multistep_table([0.0, 0.5, 1.0], "abm2").reshape(-1).tolist())
    nan = F(*good)
    nan[4] = float("nan")
    two = (C.c_float * 2)(4.0, 1.0)
    inf = float("inf")

    def call(*, coef=good, corr=1, cfg=None, rescale=0.0, limit=inf, use_cfg=1, ng=3, batch=2):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        return L.lt_sample_ode_multistep(eng.handle, P(z), P(out), P(out[4 * n:]), grid, ng, coef, corr, cfg, rescale, limit, use_cfg, 1, C.byref(a),
                                         stream())

    def masked(method):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        return L.lt_sample_ode_masked(eng.handle, P(z), P(z), P(z), P(z), P(out), P(out[4 * n:]), grid, 3, method, 1, 1, C.byref(a), stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    who = "lt_sample_ode_multistep:"
    for code in _lib.ODE_MULTISTEP_METHODS.values():
        refused(masked(code), "lt_sample_ode_masked:", "multistep method", "discontinuous")
    refused(call(corr=2), who, "corrector 2 is not 0")
    refused(call(coef=nan), who, "b[0] of interval 0 is not finite")
    refused(call(cfg=two, use_cfg=0), who, "guidance table with use_cfg = 0")
    refused(call(ng=1), who, "2 grid points")
    refused(call(cfg=(C.c_float * 2)(4.0, inf)), who, "not finite")
    refused(call(rescale=1.5), who, "rescale")
    refused(call(batch=0), "batch 0 outside")
    with pytest.raises(_lib.LuminaLibError, match="multistep method .abm2. is refused"):
        eng.sample_ode_masked(z, [0.0, 0.5, 1.0], z, z, z, "abm2", use_cfg=True)
    with pytest.raises(_lib.LuminaLibError, match="entries"):
        eng.sample_ode_multistep(z, [0.0, 0.5, 1.0], "ab2", use_cfg=True, table=[4.0])
    # ... and the same arguments untouched are served; forward_with_cfg goes on as before
    assert call(cfg=two) == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:3 * n].float()).all()) and eng.last_nfe() == 2 and eng.last_eval_rows() == 3
    assert bool(torch.isfinite(out[4 * n:5 * n].float()).all()) and torch.equal(out[2 * n:3 * n], out[4 * n:5 * n])
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0), ref)
