"""GPU: guidance reuse - lt_sample_ode_cfg_reuse / lt_forward_cfg_reuse / lt_op_unpatchify_cfg_reuse.  Everything is exact: no
tolerance.

* kernel: store mode equals lt_op_unpatchify_cfg_dev word for word and writes ``bf16(c - u)``; reuse mode equals the torch bf16 chain in both
  halves and leaves the difference alone; guard words around ``out`` and the difference buffer stay; one shape beyond a single grid pass;
* loop: the engine's trajectory equals the host loop ``transport.guidance.sample_cfg_reuse`` state for state with the row counts the tables
  imply; an all-refresh table is lt_sample_ode_cfg_schedule bit for bit;
* graph path: three keys whatever the tables hold, equal to the ``graph = 0`` run;
* one evaluation (``forward_with_cfg_reuse``) and its refusals; multistep; a class-conditional family and Flag-DiT; the C entries' refusals;
  the ``sample.py`` driver."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import EngineLimits
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

from gpu_util import P, lib, stream
from test_gpu_sde import _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
STEP_KW = dict(proportional_attn=True, base_seqlen=16)
_CACHE = {}
GUARD = 64


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- kernel --------------------------------------------------------------------------------------------------------------------------
def _kernel_case(dtype, B, H, W, eol, scales=(4.0, 1.5, 7.5, -1.0, 0.0), chs=(3, 4)):
    L = lib()
    Cc, out_ch, p = 4, 8, 2
    Hp, Wp = H // p, W // p
    stride = Wp + eol
    ws = stride if eol else 0
    ld = p * p * out_ch + 8
    half = B // 2
    g = torch.Generator().manual_seed(31 + B + 7 * eol + H)
    rows = torch.randn(B * Hp * stride, ld, generator=g).mul(3).to("cuda", torch.bfloat16)   # the refresh evaluation's final rows
    rows2 = torch.randn(half * Hp * stride, ld, generator=g).mul(3).to("cuda", torch.bfloat16)  # a reuse evaluation's: B' samples
    n = B * Cc * H * W
    code = _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32
    sentinel = 1.5

    def buf(count, dt=dtype):
        return torch.full((count + 2 * GUARD,), sentinel, dtype=dt, device="cuda")

    def guards_ok(t):
        return bool((t[:GUARD] == sentinel).all()) and bool((t[-GUARD:] == sentinel).all())

    def plain(src, b):  # the rows as a bf16 [b, C, H, W] tensor
        out = torch.empty(b * Cc * H * W, dtype=torch.bfloat16, device="cuda")
        assert L.lt_op_unpatchify_cfg(P(src), ld, P(out), _lib.LT_BF16, b, Cc, out_ch, H, W, p, 0, 1.0, 3, ws, stream()) == 0
        return out.view(b, Cc, H, W)

    o, o2 = plain(rows, B), plain(rows2, half)
    for ch in chs:
        nd = half * ch * H * W
        for scale in scales:
            tag = (dtype, B, H, W, eol, ch, scale)
            sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
            want = buf(n)
            assert L.lt_op_unpatchify_cfg_dev(P(rows), ld, P(want[GUARD:]), code, B, Cc, out_ch, H, W, p, 1, P(sc), ch, ws, 0, stream()) == 0
            got, delta = buf(n), buf(nd, torch.bfloat16)
            rc = L.lt_op_unpatchify_cfg_reuse(P(rows), ld, P(got[GUARD:]), code, B, Cc, out_ch, H, W, p, P(sc), ch, ws, P(delta[GUARD:]), 0, stream())
            assert rc == 0, L.lt_last_error()
            assert torch.equal(_bits(got), _bits(want)), tag
            d = o[:half, :ch] - o[half:, :ch]
            assert torch.equal(_bits(delta[GUARD:-GUARD]), _bits(d.reshape(-1))), tag
            assert guards_ok(got) and guards_ok(delta), tag
            # reuse: the cond rows of another evaluation, guided with the stored difference, in both halves
            kept = delta.clone()
            got = buf(n)
            rc = L.lt_op_unpatchify_cfg_reuse(P(rows2), ld, P(got[GUARD:]), code, B, Cc, out_ch, H, W, p, P(sc), ch, ws, P(delta[GUARD:]), 1, stream())
            assert rc == 0, L.lt_last_error()
            gch = (o2[:, :ch] - d) + scale * d
            r = torch.cat([gch, o2[:, ch:]], 1)
            exp = torch.cat([r, r]).to(dtype).reshape(-1)
            assert torch.equal(_bits(got[GUARD:-GUARD]), _bits(exp)), tag + (int((got[GUARD:-GUARD] != exp).sum()),)
            assert guards_ok(got) and torch.equal(_bits(delta), _bits(kept)), tag


@pytest.mark.parametrize("eol", [0, 1], ids=["grid", "eol"])
@pytest.mark.parametrize("H,W", [(4, 6), (6, 4)], ids=["4x6", "6x4"])
@pytest.mark.parametrize("B", [2, 6])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_kernel_store_and_reuse_word_for_word(dtype, B, H, W, eol):
    _kernel_case(dtype, B, H, W, eol)


def test_kernel_beyond_one_grid_pass():
    # the launcher caps its grid at 8192 blocks of 256 threads = 2 097 152 elements per pass; reuse mode walks B' C H W = 2 130 048
    assert 2 * 4 * 516 * 516 > 8192 * 256
    _kernel_case(torch.bfloat16, 4, 516, 516, 1, scales=(4.0,), chs=(3,))


def test_kernel_refusals():
    L = lib()
    rows = torch.zeros(2 * 6, 40, dtype=torch.bfloat16, device="cuda")
    out = torch.full((2 * 4 * 4 * 6,), float("nan"), dtype=torch.bfloat16, device="cuda")
    delta = torch.full((4 * 4 * 6,), float("nan"), dtype=torch.bfloat16, device="cuda")
    sc = torch.tensor([4.0], device="cuda")

    def call(B=2, ch=3, mode=0, d=delta, s=sc):
        return L.lt_op_unpatchify_cfg_reuse(P(rows), 40, P(out), _lib.LT_BF16, B, 4, 8, 4, 6, 2, P(s), ch, 0, P(d), mode, stream())

    for k, word in ((dict(B=3), "even count"), (dict(ch=0), "cfg_channels"), (dict(ch=5), "cfg_channels"), (dict(mode=2), "mode 2"),
                    (dict(d=None), "null argument"), (dict(s=None), "null argument")):
        rc = call(**k)
        msg = L.lt_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg, word)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(delta).all())


# ---- loop ----------------------------------------------------------------------------------------------------------------------------
def _next(golden_dir):
    if "next" not in _CACHE:
        model, z, kw = _model(golden_dir, "next")
        _CACHE["next"] = (model, kw)
    return _CACHE["next"]


def _grid(method):
    return ODE(5, method, 4).t  # a 5-point shifted grid: 4 / 8 / 16 evaluations


def _mixed(method):
    """(scales, flags): refresh, reuse and scale-1 stages, reuse stages at another scale than their refresh, a flag 1 at scale 1"""
    n = 4 * STAGES[method]
    scales = [4.0, 3.0, 1.0, 2.5, 4.0, 1.0, 5.0, 1.5, 4.0, 4.0, 1.0, 2.0, 3.5, 3.0, 1.0, 4.0][:n]
    flags = [0, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 1, 1, 1][:n]
    if n == 4:
        scales, flags = [4.0, 3.0, 1.0, 2.5], [0, 1, 1, 1]
    return torch.tensor(scales), torch.tensor(flags, dtype=torch.int32)


def _counts(scales, flags):
    guided = scales != 1
    refresh = int((guided & (flags == 0)).sum())
    return refresh, int(guided.sum()) - refresh, int((~guided).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    tgrid = _grid(method)
    scales, flags = _mixed(method)
    Gn, Rn, Cn = _counts(scales, flags)
    assert Gn > 0 and Rn > 0 and Cn > 0
    g = torch.Generator().manual_seed(6)
    for B, H, W in ((2, 16, 16), (4, 16, 24)):
        Bh = B // 2
        tag = (method, dtype, B)
        z = torch.randn(Bh, 4, H, W, generator=g).to("cuda", dtype).repeat(2, 1, 1, 1)
        cf, cm = (cap, cmask) if B == 2 else (torch.cat([cap, cap.flip(0)]), torch.cat([cmask, cmask.flip(0)]))
        model.forward_with_cfg(z, torch.zeros(B, device="cuda"), cf, cm, 4.0, **STEP_KW)  # the flags a plain forward reads
        got = model.sample_ode_cfg_schedule(z, tgrid, scales, cf, cm, method=method, return_trajectory=True, reuse=flags, **STEP_KW)
        eng = model._engine
        assert eng.last_nfe() == len(scales) and eng.last_eval_rows() == B * Gn + Bh * (Rn + Cn), tag + (eng.last_nfe(), eng.last_eval_rows())
        want = G.sample_cfg_reuse(model, z, tgrid, scales, flags, method, cap_feats=cf, cap_mask=cm, **STEP_KW)
        assert got.shape == want.shape == (len(tgrid),) + tuple(z.shape) and got.dtype == dtype, tag
        assert bool(torch.isfinite(want.float()).all()), tag
        for i in range(len(tgrid)):
            assert torch.equal(got[i], want[i]), tag + (i, int((got[i] != want[i]).sum()))
        final = model.sample_ode_cfg_schedule(z, tgrid, scales, cf, cm, method=method, reuse=flags, **STEP_KW)
        assert torch.equal(final, got[-1]), tag
        # the reuse stages are not what full guidance computes
        full = model.sample_ode_cfg_schedule(z, tgrid, scales, cf, cm, method=method, return_trajectory=True, **STEP_KW)
        assert not torch.equal(full[-1], got[-1]), tag
        # an all-refresh table is the schedule call, bit for bit
        zeros = model.sample_ode_cfg_schedule(z, tgrid, scales, cf, cm, method=method, return_trajectory=True, reuse=torch.zeros_like(flags),
                                              **STEP_KW)
        assert eng.last_eval_rows() == B * (Gn + Rn) + Bh * Cn, tag
        assert torch.equal(zeros, full), tag
        # through the transport front end: the same call, and the host loop with use_engine = False
        o = ODE(len(tgrid), method, 4)
        via = o.sample(z, model.forward_with_cfg, cfg_table=scales, cfg_reuse=flags, cap_feats=cf, cap_mask=cm, cfg_scale=4.0, **STEP_KW)
        assert torch.equal(via, got), tag


def test_graph_path_replays_three_keys_whatever_the_tables(golden_dir):
    model, _, kw = _model(golden_dir, "next")  # a fresh engine: no key has been used
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    H, W = 50, 82  # 25 x 41 = 1025 tokens: the smallest latent whose B' = 1 evaluation has more than 1024 rows
    assert (H // 2) * (W // 2) == 1025
    tgrid = ODE(7, "midpoint", 4).t  # 12 evaluations
    scales = torch.tensor([2.0, 3.0, 1.0, 3.5, 4.5, 1.0, 5.0, 2.0, 2.5, 1.0, 4.0, 3.0])
    flags = torch.tensor([0, 1, 0, 1, 0, 1, 1, 1, 0, 0, 0, 1], dtype=torch.int32)
    Gn, Rn, Cn = _counts(scales, flags)
    assert (Gn, Rn, Cn) == (4, 5, 3)
    z = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(8)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), cap, cmask, 4.0, **STEP_KW)  # engine, weights, prompt
    eng = model._engine
    before = eng.graph_replays()
    got = model.sample_ode_cfg_schedule(z, tgrid, scales, cap, cmask, method="midpoint", return_trajectory=True, reuse=flags, **STEP_KW)
    # the first use of a key runs eagerly, every later one replays: neither the scale nor the place in the tables is part of a key
    assert eng.graph_replays() - before == (Gn - 1) + (Rn - 1) + (Cn - 1)
    assert eng.last_nfe() == 12 and eng.last_eval_rows() == 2 * Gn + Rn + Cn
    assert eng.get_option("layout_flips") >= 0
    again = model.sample_ode_cfg_schedule(z, tgrid, scales, cap, cmask, method="midpoint", return_trajectory=True, reuse=flags, **STEP_KW)
    assert eng.graph_replays() - before == 2 * 12 - 3 and torch.equal(again, got)
    eng.set_option("graph", 0)
    try:
        eager = model.sample_ode_cfg_schedule(z, tgrid, scales, cap, cmask, method="midpoint", return_trajectory=True, reuse=flags, **STEP_KW)
        assert eng.graph_replays() - before == 2 * 12 - 3
    finally:
        eng.set_option("graph", None)
    for i in range(len(tgrid)):
        assert torch.equal(got[i], eager[i]), (i, int((got[i] != eager[i]).sum()))


# ---- one evaluation ------------------------------------------------------------------------------------------------------------------
def test_forward_with_cfg_reuse_stores_reuses_and_refuses_by_name(golden_dir):
    model, _, kw = _model(golden_dir, "next")  # a fresh engine: nothing is stored
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    g = torch.Generator().manual_seed(12)
    for dtype in DTYPES:
        z = torch.randn(1, 4, 16, 16, generator=g).to("cuda", dtype).repeat(2, 1, 1, 1)
        z2 = torch.randn(1, 4, 16, 16, generator=g).to("cuda", dtype).repeat(2, 1, 1, 1)
        t, t2 = torch.full((2,), 0.25, device="cuda"), torch.full((2,), 0.5, device="cuda")
        ref = model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
        eng = model._engine
        nan = torch.full_like(z, float("nan"))

        def refused(words, **k):
            out = nan.clone()
            with pytest.raises(_lib.LuminaLibError) as exc:
                eng.forward_cfg_reuse(k.pop("x", z2), t2, cfg_scale=2.5, reuse=True, out=out, **STEP_KW, **k)
            assert all(w in str(exc.value) for w in words), str(exc.value)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all())

        if dtype == DTYPES[0]:
            refused(("lt_forward_cfg_reuse:", "no stored"))
        got = model.forward_with_cfg_reuse(z, t, cap, cmask, 4.0, **STEP_KW)
        assert torch.equal(got, ref), dtype
        # the host expressions: d from the plain forward of both halves, the reuse chain on the cond row of another state at another scale
        o = model.forward(z, t, cap, cmask).to(torch.bfloat16)
        d = o[:1, :3] - o[1:, :3]
        assert torch.equal(got, torch.cat([torch.cat([o[1:, :3] + 4.0 * d] * 2), o[:, 3:]], 1).to(dtype)), dtype
        model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)  # (the prompt of both rows again, the flags: the plain forward left its own)
        eng.forward_cfg_reuse(z, t, cfg_scale=4.0, reuse=False, **STEP_KW)
        got2 = model.forward_with_cfg_reuse(z2, t2, cap, cmask, 2.5, reuse=True, **STEP_KW)
        c2 = model.forward(z2[:1], t2[:1], cap[:1].contiguous(), cmask[:1].contiguous()).to(torch.bfloat16)
        r = torch.cat([(c2[:, :3] - d) + 2.5 * d, c2[:, 3:]], 1)
        assert torch.equal(got2, torch.cat([r, r]).to(dtype)), dtype
        # a prepare call forgets the difference; so does another latent size
        model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
        refused(("lt_forward_cfg_reuse:", "no stored"))
        eng.forward_cfg_reuse(z, t, cfg_scale=4.0, reuse=False, **STEP_KW)
        eng.forward_cfg_reuse(z2, t2, cfg_scale=2.5, reuse=True, **STEP_KW)
        eng.prepare_prompt(cap.clone(), cmask.clone())
        refused(("lt_forward_cfg_reuse:", "lt_prepare_prompt"))
        eng.forward_cfg_reuse(z, t, cfg_scale=4.0, reuse=False, **STEP_KW)
        nan = torch.full((2, 4, 16, 8), float("nan"), dtype=dtype, device="cuda")
        refused(("lt_forward_cfg_reuse:", "another shape"), x=torch.zeros_like(nan))
        nan = torch.full_like(z, float("nan"))
        assert torch.equal(eng.forward_cfg_reuse(z2, t2, cfg_scale=2.5, reuse=True, **STEP_KW), got2), dtype
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.forward_with_cfg_reuse([z[:1], z[:1]], t, cap, cmask, 4.0)


# ---- multistep -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["abm2", "ab3"])
def test_multistep_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    tgrid = ODE(7, "euler", 4).t
    scales = torch.tensor([4.0, 3.0, 1.0, 2.5, 4.0, 3.5])
    flags = torch.tensor([0, 1, 1, 1, 0, 1], dtype=torch.int32)
    z = torch.randn(1, 4, 16, 24, generator=torch.Generator().manual_seed(21)).to("cuda", dtype).repeat(2, 1, 1, 1)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), cap, cmask, 4.0, **STEP_KW)
    got = model.sample_ode_cfg_schedule(z, tgrid, scales, cap, cmask, method=method, return_trajectory=True, reuse=flags, **STEP_KW)
    eng = model._engine
    assert eng.last_nfe() == 6 and eng.last_eval_rows() == 2 * 2 + 3 + 1
    want = G.sample_cfg_reuse_multistep(model, z, tgrid, scales, flags, method, cap_feats=cap, cap_mask=cmask, **STEP_KW)
    assert got.shape == want.shape and bool(torch.isfinite(want.float()).all())
    for i in range(len(tgrid)):
        assert torch.equal(got[i], want[i]), (method, dtype, i, int((got[i] != want[i]).sum()))
    o = ODE(7, method, 4)
    assert torch.equal(o.sample(z, model.forward_with_cfg, cfg_table=scales, cfg_reuse=flags, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0,
                                **STEP_KW), got)


@pytest.mark.parametrize("family", ["imagenet", "flag"])
def test_other_families_run_the_same_call_through_the_transport_front_end(golden_dir, family):
    model, z, kw = _model(golden_dir, family)
    z = z.to("cuda", torch.bfloat16)
    assert z.shape[0] == 2
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), **kw)  # the flags a plain forward reads
    o = ODE(5, "midpoint", 4)
    scales = torch.tensor([1.0, 2.0, 2.0, 1.0, 4.0, 3.0, 3.0, 1.0])
    flags = torch.tensor([0, 0, 1, 0, 0, 1, 1, 1], dtype=torch.int32)
    got = o.sample(z, model.forward_with_cfg, cfg_table=scales, cfg_reuse=flags, **kw)
    assert model._engine.last_nfe() == 8 and model._engine.last_eval_rows() == 2 * 2 + 3 + 3
    o.use_engine = False
    want = o.sample(z, model.forward_with_cfg, cfg_table=scales, cfg_reuse=flags, **kw)
    assert got.shape == (5,) + tuple(z.shape) and bool(torch.isfinite(want.float()).all())
    for i in range(5):
        assert torch.equal(got[i], want[i]), (family, i, int((got[i] != want[i]).sum()))
    with pytest.raises(ValueError, match="rescale / norm_limit"):
        o.sample(z, model.forward_with_cfg, cfg_table=scales, cfg_reuse=flags, cfg_rescale=0.5, **kw)
    o.use_engine = True
    with pytest.raises(ValueError, match="rescale / norm_limit"):
        o.sample(z, model.forward_with_cfg, cfg_table=scales, cfg_reuse=flags, cfg_norm_limit=1.5, **kw)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    n = 2 * 4 * 16 * 16
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    lim = model.engine_limits  # room for a batch of 3: the odd batch must reach its own refusal
    model.engine_limits = EngineLimits(max(lim.max_batch, 6), lim.max_tokens, lim.max_text)
    t = torch.full((2,), 0.5, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0)  # engine, weights, a prompt of 2 rows
    eng, L = model._engine, lib()
    out = torch.full((8 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    grid = (C.c_float * 4)(0.0, 0.25, 0.5, 1.0)
    good, bad = (C.c_float * 3)(4.0, 1.0, 3.0), (C.c_float * 3)(4.0, float("nan"), 3.0)
    i32 = C.c_int32 * 3
    from lumina_t2x_amd.transport.multistep import multistep_table
    coef = multistep_table(torch.tensor([0.0, 0.25, 0.5, 1.0]), "abm2").contiguous()

    def call(*, tab=good, flg=i32(0, 1, 1), method=0, ng=4, batch=2, zz=P(z), multistep=False):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        if multistep:
            return L.lt_sample_ode_multistep_cfg_reuse(eng.handle, zz, P(out), P(out[4 * n:]), grid, ng, C.cast(coef.data_ptr(), C.POINTER(C.c_float)),
                                                       1, tab, flg, 1, C.byref(a), stream())
        return L.lt_sample_ode_cfg_reuse(eng.handle, zz, P(out), P(out[4 * n:]), grid, ng, method, tab, flg, 1, C.byref(a), stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    for ms, who in ((False, "lt_sample_ode_cfg_reuse:"), (True, "lt_sample_ode_multistep_cfg_reuse:")):
        refused(call(batch=3, multistep=ms), who, "even batch")
        refused(call(tab=bad, multistep=ms), who, "not finite")
        refused(call(ng=1, multistep=ms), who, "2 grid points")
        refused(call(tab=None, multistep=ms), who, "null argument")
        refused(call(flg=None, multistep=ms), who, "null argument", "reuse_host")
        refused(call(zz=C.c_void_p(0), multistep=ms), who, "null argument")
        refused(call(flg=i32(0, 1, 2), multistep=ms), who, "reuse flag 2 of evaluation 2")
        refused(call(flg=i32(0, 1, -1), multistep=ms), who, "reuse flag -1")
        refused(call(flg=i32(1, 0, 0), multistep=ms), who, "evaluation 0 reuses", "no refresh")
        # a flag 1 at scale 1 is no reuse: the first guided evaluation is number 2 here
        refused(call(tab=(C.c_float * 3)(1.0, 1.0, 3.0), flg=i32(0, 0, 1), multistep=ms), who, "evaluation 2 reuses")
        refused(call(batch=0, multistep=ms), "batch 0 outside")
    refused(call(method=7), "lt_sample_ode_cfg_reuse:", "unknown method")
    # a stream under capture: refused before anything is launched, the caller's capture stays valid and its other content replays
    a = torch.arange(64, dtype=torch.float32, device="cuda")
    graph, side, seen = torch.cuda.CUDAGraph(), torch.cuda.Stream(), []
    with torch.cuda.graph(graph, stream=side):
        for ms in (False, True):
            seen.append((call(multistep=ms), L.lt_last_error().decode()))
        b = a + 1.0
    for (rc, msg), who in zip(seen, ("lt_sample_ode_cfg_reuse:", "lt_sample_ode_multistep_cfg_reuse:")):
        assert rc != 0 and who in msg and "capture" in msg, (rc, msg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(b, a + 1.0) and bool(torch.isnan(out).all())
    eng.prepare_prompt_regional(cap, cmask, cap[:1].contiguous(), cmask[:1].contiguous(), 1, 1)
    refused(call(), "lt_sample_ode_cfg_reuse:", "regional prompt")
    with pytest.raises(_lib.LuminaLibError, match="entries"):
        eng.sample_ode_cfg_reuse(z, [0.0, 0.5, 1.0], [4.0, 4.0], [0], "euler")
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        eng.sample_ode_cfg_reuse([z[:1], z[:1]], [0.0, 0.5, 1.0], [4.0, 4.0], [0, 1], "euler")
    with pytest.raises(_lib.LuminaLibError, match="rescale / norm_limit"):
        model.sample_ode_cfg_schedule(z, [0.0, 0.5, 1.0], [4.0, 4.0], cap, cmask, method="euler", reuse=[0, 1], rescale=0.5)
    # ... and the same arguments untouched are served, with the prompt prepared ONCE for both rows; forward_with_cfg goes on as before
    eng.prepare_prompt(cap, cmask)
    assert call() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:4 * n].float()).all()) and eng.last_nfe() == 3 and eng.last_eval_rows() == 2 + 1 + 1
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0), ref)


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_sample_driver_with_cfg_reuse_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_reuse_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_reuse_test"] = ctor
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

    argv = ["--ckpt", str(ck), "--caption_path", str(tmp_path / "prompts.txt"), "--resolution", "256:128x128", "--num_sampling_steps", "5",
            "--sampling-method", "midpoint", "--time_shifting_factor", "4", "--seed", "11"]
    runs = {}
    try:
        for name, extra in (("default", []), ("every2", ["--cfg_reuse", "2"]), ("per_step", ["--cfg_reuse_per_step"]),
                            ("interval", ["--cfg_reuse", "2", "--cfg_interval", "0.1", "0.8"])):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            runs[name] = (built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
        with pytest.raises(SystemExit, match="cfg_rescale"):
            S.run(S.build_parser().parse_args(argv + ["--cfg_reuse", "2", "--cfg_rescale", "0.5", "--image_save_path", str(tmp_path / "no")]),
                  encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
    finally:
        del models.__dict__["NextDiT_tiny_reuse_test"]
    fn = Sampler(create_transport()).sample_ode(sampling_method="midpoint", num_steps=5, time_shifting_factor=4.0)
    tgrid = fn.__self__.t
    itab = G.cfg_table(tgrid, "midpoint", 4.0, interval=(0.1, 0.8))
    Gi, Ci = int((itab != 1).sum()), int((itab == 1).sum())
    assert Gi > 1 and Ci > 0
    # every evaluation of a run lies in ONE whole-trajectory call; the reuse stages run one row: fewer rows than full guidance
    assert runs == {"default": (8, 16), "every2": (8, 12), "per_step": (8, 12), "interval": (8, 2 * ((Gi + 1) // 2) + Gi // 2 + Ci)}
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    feats, mask = encode(["a red cube", ""])
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    # the default invocation is the call it was
    want = fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1]
    assert torch.equal(decoded[0], want / 0.13025)
    fours = torch.full((8,), 4.0)
    want = model.sample_ode_cfg_schedule(z, tgrid, fours, feats, mask, method="midpoint", reuse=[0, 1] * 4, **kw)[:1]
    assert torch.equal(decoded[1], want / 0.13025) and not torch.equal(decoded[1], decoded[0])
    assert torch.equal(decoded[2], decoded[1])  # (midpoint: every second guided stage IS the step's second stage)
    want = model.sample_ode_cfg_schedule(z, tgrid, itab, feats, mask, method="midpoint",
                                         reuse=G.cfg_reuse_table(tgrid, "midpoint", itab, every=2), **kw)[:1]
    assert torch.equal(decoded[3], want / 0.13025) and not torch.equal(decoded[3], decoded[0])
