"""GPU: prompt-driven editing - lt_sample_flowedit / lt_op_flowedit_mix / lt_op_flowedit_combine (FlowEdit).  Everything is exact: no
tolerance.

* kernels: both equal the torch expressions of transport/edit.py run on the device and the float64 restatement (tests/exact_edit.py) word for
  word, at bf16 and fp32, B' = 1 and 2, ch = 3 of 4 and ch = C, sizes that are no multiple of the block, one shape beyond a single grid pass,
  ``x_src`` aliasing ``z``, the tie operands; guard words around every output stay;
* loop: ``model.sample_flowedit`` equals ``transport.edit.sample_flowedit`` around the same model's plain ``forward`` at every slot, for three
  families, with the evaluation and row counts the header states;
* graph path: one key, equal to the ``graph = 0`` run; identical conditioning keeps the source; the C entry's refusals; the driver."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import DiTEngine, EngineLimits
from lumina_t2x_amd.transport import edit as E
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

import exact_edit as X
from gpu_util import P, lib, stream
from test_gpu_sde import _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
STEP_KW = dict(proportional_attn=True, base_seqlen=16)
GUARD = 64
SENTINEL = 1.5


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _code(dtype):
    return _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32


def _buf(count, dtype):
    return torch.full((count + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")


def _guards_ok(t):
    return bool((t[:GUARD] == SENTINEL).all()) and bool((t[-GUARD:] == SENTINEL).all())


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
def _mix(x, z, w, t, omt):
    n = x.numel()
    out = _buf(4 * n, x.dtype)
    rc = lib().lt_op_flowedit_mix(P(x), P(z), P(w), P(out[GUARD:]), t, omt, n, _code(x.dtype), stream())
    assert rc == 0, lib().lt_last_error()
    return out


def _combine(z, out4, w_s, w_t, dt, Bp, Cc, HW, ch, into=None):
    n = Bp * Cc * HW
    out = _buf(n, z.dtype)
    rc = lib().lt_op_flowedit_combine(P(z), P(out4), P(out[GUARD:] if into is None else into), w_s, w_t, dt, Bp, Cc, HW, ch, _code(z.dtype), stream())
    assert rc == 0, lib().lt_last_error()
    return out


def _operands(dtype, Bp, Cc, HW, seed):
    g = torch.Generator().manual_seed(seed)
    x, w = (torch.randn(Bp, Cc, 1, HW, generator=g).to("cuda", dtype) for _ in range(2))
    z = (x.float().cpu() + 0.05 * torch.randn(Bp, Cc, 1, HW, generator=g)).to("cuda", dtype)
    out4 = torch.randn(4 * Bp, Cc, 1, HW, generator=g).mul(1.5).to("cuda", dtype)
    return x, z, w, out4


def _check_mix(x, z, w, t, t1, tag, f64=True):
    tt, omt, _ = X.scalars(t, t1)
    got = _mix(x, z, w, float(tt), float(omt))
    zs, zt = E.mix(x, z, w, float(tt))
    want = torch.cat([zs, zt, zs, zt]).reshape(-1)
    assert _guards_ok(got), tag
    assert torch.equal(_bits(got[GUARD:-GUARD]), _bits(want)), tag + (int((got[GUARD:-GUARD] != want).sum()),)
    if f64:
        ws, wt = X.mix_chain(X.f64(x), X.f64(z), X.f64(w), tt, omt, X.rounding(x.dtype))
        assert X.same_words(got[GUARD:-GUARD], np.concatenate([ws, wt, ws, wt]).reshape(-1)), tag


def _check_combine(z, out4, w_s, w_t, t, t1, ch, tag, f64=True):
    Bp, Cc, HW = z.shape[0], z.shape[1], z.shape[2] * z.shape[3]
    _, _, dt = X.scalars(t, t1)
    got = _combine(z, out4, w_s, w_t, float(dt), Bp, Cc, HW, ch)
    want = E.combine(z, out4, w_s, w_t, float(np.float32(t1)) - float(np.float32(t)), ch).reshape(-1)
    assert _guards_ok(got), tag
    assert torch.equal(_bits(got[GUARD:-GUARD]), _bits(want)), tag + (int((got[GUARD:-GUARD] != want).sum()),)
    if f64:
        w64 = X.combine_chain(X.f64(z), X.f64(out4), w_s, w_t, dt, ch, X.rounding(z.dtype))
        assert X.same_words(got[GUARD:-GUARD], w64.reshape(-1)), tag


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_kernels_equal_the_torch_expressions_and_the_float64_chain_word_for_word(dtype):
    grid = ODE(6, "euler", 4).t
    t, t1 = float(grid[2]), float(grid[3])
    # mix: a flat size that is no multiple of the block or of a vector, B' = 1 and 2 of the combine shapes
    for shape in ((1, 1, 4097), (1, 4, 1025), (2, 4, 1025), (1, 4, 3)):
        x, z, w, _ = _operands(dtype, *shape, seed=sum(shape))
        _check_mix(x, z, w, t, t1, ("mix", dtype, shape))
        _check_mix(x, x, w, t, t1, ("mix alias", dtype, shape))  # x_src aliasing z: zt == zs
        got = _mix(x, x, w, t, float(np.float32(1.0 - t)))
        n = x.numel()
        assert torch.equal(_bits(got[GUARD:GUARD + n]), _bits(got[GUARD + n:GUARD + 2 * n]))
    for Bp in (1, 2):
        for ch in (3, 4):
            for w_s, w_t in ((1.5, 5.5), (1.0, 1.0), (0.0, -2.25)):
                x, z, w, out4 = _operands(dtype, Bp, 4, 1025, seed=10 * Bp + ch)
                _check_combine(z, out4, w_s, w_t, t, t1, ch, ("combine", dtype, Bp, ch, w_s, w_t))
    # the tie operands: w d, v_t - v_s and the final sum between two bf16 values
    z, out4, w_s, w_t, dtf, ch = X.tie_operands(dtype)
    _check_combine(z.cuda(), out4.cuda(), w_s, w_t, 0.25, 0.5, ch, ("combine ties", dtype))
    x, z, w, tq = X.mix_tie_operands(dtype)
    _check_mix(x.cuda(), z.cuda(), w.cuda(), tq, 0.5, ("mix ties", dtype))
    # z_next aliasing z: every thread reads its element before it writes it
    x, z, w, out4 = _operands(dtype, 2, 4, 1025, seed=77)
    want = E.combine(z, out4, 1.5, 5.5, t1 - t, 3)
    _combine(z, out4, 1.5, 5.5, float(np.float32(t1 - t)), 2, 4, 1025, 3, into=z)
    assert torch.equal(_bits(z), _bits(want))


def test_kernels_beyond_one_grid_pass():
    n = 8192 * 256 + 257  # the launchers cap the grid at 8192 blocks of 256 threads
    g = torch.Generator(device="cuda").manual_seed(5)
    x, w = (torch.randn(1, 1, 1, n, generator=g, device="cuda").to(torch.bfloat16) for _ in range(2))
    z = (x.float() + 0.05 * torch.randn(1, 1, 1, n, generator=g, device="cuda")).to(torch.bfloat16)
    _check_mix(x, z, w, 0.3, 0.45, ("mix big",), f64=False)
    out4 = torch.randn(4, 1, 1, n, generator=g, device="cuda").mul(1.5).to(torch.bfloat16)
    _check_combine(z, out4, 1.5, 5.5, 0.3, 0.45, 1, ("combine big",), f64=False)


def test_kernel_refusals_leave_the_outputs_untouched():
    L = lib()
    x = torch.zeros(1, 4, 1, 8, dtype=torch.bfloat16, device="cuda")
    out4 = torch.full((4 * 32,), float("nan"), dtype=torch.bfloat16, device="cuda")
    zn = torch.full((32,), float("nan"), dtype=torch.bfloat16, device="cuda")

    def mix(xs=x, z=x, w=x, o=out4, n=32, code=_lib.LT_BF16):
        return L.lt_op_flowedit_mix(P(xs), P(z), P(w), P(o), 0.5, 0.5, n, code, stream())

    def comb(z=x, o=out4, nxt=zn, Bp=1, Cc=4, HW=8, ch=3, code=_lib.LT_BF16):
        return L.lt_op_flowedit_combine(P(z), P(o), P(nxt), 1.5, 5.5, 0.1, Bp, Cc, HW, ch, code, stream())

    for rc_of, word in ((lambda: mix(xs=None), "null argument"), (lambda: mix(z=None), "null argument"), (lambda: mix(w=None), "null argument"),
                        (lambda: mix(o=None), "null argument"), (lambda: mix(code=_lib.LT_F16), "state dtype"), (lambda: mix(n=0), "elements"),
                        (lambda: mix(n=-3), "elements"),
                        (lambda: comb(z=None), "null argument"), (lambda: comb(o=None), "null argument"), (lambda: comb(nxt=None), "null argument"),
                        (lambda: comb(code=3), "state dtype"), (lambda: comb(Bp=0), "at least 1"), (lambda: comb(HW=0), "at least 1"),
                        (lambda: comb(Cc=-1), "at least 1"), (lambda: comb(ch=0), "cfg_channels"), (lambda: comb(ch=5), "cfg_channels"),
                        (lambda: comb(nxt=out4[32:]), "inside the evaluation"), (lambda: comb(nxt=out4[3 * 32 + 31:]), "inside the evaluation")):
        rc = rc_of()
        msg = L.lt_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg, word)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out4).all()) and bool(torch.isnan(zn).all())


# ---- loop ----------------------------------------------------------------------------------------------------------------------------
def _cond(family, kw, Bp, seed=2):
    """the conditioning of 4 B' rows [src_*, tgt_*, neg_src_*, neg_tgt_*] from a fixture's (cond, uncond) pair"""
    if family == "imagenet":
        y0, null = int(kw["y"][0]), int(kw["y"][1])
        src = [(y0 + b) % null for b in range(Bp)]
        tgt = [(y0 + 1 + Bp + b) % null for b in range(Bp)]
        return (torch.tensor(src + tgt + [null] * (2 * Bp), device="cuda"),)
    cap, mask = kw["cap_feats"], kw["cap_mask"]
    g = torch.Generator().manual_seed(seed)
    src = torch.cat([cap[:1]] + [torch.randn(cap[:1].shape, generator=g).to("cuda", cap.dtype) for _ in range(Bp - 1)])
    tgt = torch.randn((Bp,) + tuple(cap.shape[1:]), generator=g).to("cuda", cap.dtype)
    neg = cap[1:].expand(2 * Bp, -1, -1)
    feats = torch.cat([src, tgt, neg]).contiguous()
    masks = torch.cat([mask[:1].expand(2 * Bp, -1), mask[1:].expand(2 * Bp, -1)]).contiguous()
    return feats, masks


def _host(model, x, tgrid, noise, scales, cond, z=None):
    names = model._cond_names
    return E.sample_flowedit(model.forward, x, tgrid, noise, scales, z=z, **dict(zip(names, cond)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("family", ["next", "imagenet", "flag"])
def test_engine_trajectory_equals_the_host_loop_at_every_slot(golden_dir, family, dtype):
    model, _, kw = _model(golden_dir, family)
    step_kw = STEP_KW if family != "imagenet" else {}
    g = torch.Generator().manual_seed(6)
    cases = (  # grid, B', H, W, src_cfg, tgt_cfg
        (ODE(5, "euler", 4).t, 1, 16, 16, 1.5, 5.5),                                            # a 5-point shifted grid, constant scales
        (ODE(10, "euler", 4, strength=0.6).t, 2, 16, 24, [1.0, 1.5, 2.0, 1.25, 0.0], [5.5, 4.5, 1.0, 3.5, 6.0]),  # a cut grid, a table per interval
    )
    for tgrid, Bp, H, W, sw, tw in cases:
        n = len(tgrid) - 1
        tag = (family, dtype, Bp)
        x = torch.randn(Bp, 4, H, W, generator=g).to("cuda", dtype)
        noise = torch.randn(n, Bp, 4, H, W, generator=g).to("cuda", dtype)
        cond = _cond(family, kw, Bp)
        got = model.sample_flowedit(x, tgrid, noise, *cond, src_cfg=sw, tgt_cfg=tw, return_trajectory=True, **step_kw)
        eng = model._engine
        assert eng.last_nfe() == n and eng.last_eval_rows() == 4 * Bp * n, tag + (eng.last_nfe(), eng.last_eval_rows())
        scales = E.flowedit_scales(n, sw, tw)
        want = _host(model, x, tgrid, noise, scales, cond)
        assert got.shape == want.shape == (n + 1,) + tuple(x.shape) and got.dtype == dtype, tag
        assert bool(torch.isfinite(want.float()).all()) and not torch.equal(want[-1], x), tag
        for i in range(n + 1):
            assert torch.equal(got[i], want[i]), tag + (i, int((got[i] != want[i]).sum()))
        final = model.sample_flowedit(x, tgrid, noise, *cond, src_cfg=sw, tgt_cfg=tw, **step_kw)
        assert torch.equal(final, got[-1]), tag
        # an edit state other than the source (the hand-over of a second call): the same equality
        z = got[2]
        got2 = model.sample_flowedit(x, tgrid[2:], noise[2:], *cond, src_cfg=scales[2:, 0], tgt_cfg=scales[2:, 1], z=z, return_trajectory=True, **step_kw)
        for i in range(n - 1):
            assert torch.equal(got2[i], got[2 + i]), tag + ("from slot 2", i)


def test_graph_path_replays_one_key_and_equals_the_eager_run(golden_dir):
    model, _, kw = _model(golden_dir, "next")  # a fresh engine: no key has been used
    H, W = 34, 32  # 17 x 16 = 272 tokens: 4 x 272 = 1088 rows, more than 1024
    assert 4 * (H // 2) * (W // 2) > 1024
    cond = _cond("next", kw, 1)
    model.engine_limits = EngineLimits(4, 272, cond[0].shape[1])
    tgrid = ODE(6, "euler", 4).t
    n = 5
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 4, H, W, generator=g).to("cuda", torch.bfloat16)
    noise = torch.randn(n, 1, 4, H, W, generator=g).to("cuda", torch.bfloat16)
    model.forward(x, torch.zeros(1, device="cuda"), cond[0][:1].contiguous(), cond[1][:1].contiguous())  # engine and weights; 272 rows: no graph
    eng = model._engine
    before = eng.graph_replays()
    got = model.sample_flowedit(x, tgrid, noise, *cond, src_cfg=[1.0, 1.5, 2.0, 1.5, 1.0], tgt_cfg=[5.5, 4.5, 3.5, 2.5, 6.5], return_trajectory=True, **STEP_KW)
    assert model._engine is eng
    # the first use of the key runs eagerly, every later one replays: neither the scales nor the interval are part of it
    assert eng.graph_replays() - before == n - 1
    assert eng.last_nfe() == n and eng.last_eval_rows() == 4 * n
    again = model.sample_flowedit(x, tgrid, noise, *cond, src_cfg=[1.0, 1.5, 2.0, 1.5, 1.0], tgt_cfg=[5.5, 4.5, 3.5, 2.5, 6.5], return_trajectory=True, **STEP_KW)
    assert eng.graph_replays() - before == 2 * n - 1 and torch.equal(again, got)
    eng.set_option("graph", 0)
    try:
        eager = model.sample_flowedit(x, tgrid, noise, *cond, src_cfg=[1.0, 1.5, 2.0, 1.5, 1.0], tgt_cfg=[5.5, 4.5, 3.5, 2.5, 6.5], return_trajectory=True,
                                      **STEP_KW)
        assert eng.graph_replays() - before == 2 * n - 1
    finally:
        eng.set_option("graph", None)
    for i in range(n + 1):
        assert torch.equal(got[i], eager[i]), (i, int((got[i] != eager[i]).sum()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_identical_conditioning_with_equal_scales_equals_the_host_loop(golden_dir, dtype):
    model, _, kw = _model(golden_dir, "next")
    cap, mask = kw["cap_feats"], kw["cap_mask"]
    feats = torch.cat([cap[:1], cap[:1], cap[1:], cap[1:]]).contiguous()  # source == target, one negative prompt
    masks = torch.cat([mask[:1], mask[:1], mask[1:], mask[1:]]).contiguous()
    tgrid = ODE(5, "euler", 4).t
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 4, 16, 16, generator=g).to("cuda", dtype)
    noise = torch.randn(4, 1, 4, 16, 16, generator=g).to("cuda", dtype)
    got = model.sample_flowedit(x, tgrid, noise, feats, masks, src_cfg=3.5, tgt_cfg=3.5, return_trajectory=True, **STEP_KW)
    want = E.sample_flowedit(model.forward, x, tgrid, noise, E.flowedit_scales(4, 3.5, 3.5), cap_feats=feats, cap_mask=masks)
    for i in range(5):
        assert torch.equal(got[i], want[i]), (dtype, i)
        if torch.equal(want[i], x):  # rows with one input and one conditioning: where the model returns one output for them, nothing moves
            assert torch.equal(got[i], x), (dtype, i)
    assert torch.equal(want[0], x) and torch.equal(got[0], x)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    model, _, kw = _model(golden_dir, "next")
    feats, masks = _cond("next", kw, 1)
    lim = model.engine_limits  # room for 8 rows: a batch of 6 must reach its own refusal, one of 8 the prompt's
    model.engine_limits = EngineLimits(max(lim.max_batch, 8), max(lim.max_tokens, 64), max(lim.max_text, feats.shape[1]))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 16, 16, generator=g).to("cuda", torch.bfloat16)
    noise = torch.randn(3, 1, 4, 16, 16, generator=g).to("cuda", torch.bfloat16)
    n = x.numel()
    ref = model.sample_flowedit(x, [0.0, 0.25, 0.5, 1.0], noise, feats, masks, src_cfg=1.5, tgt_cfg=5.5)  # engine, weights, a prompt of 4 rows
    eng, L = model._engine, lib()
    out = torch.full((5 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    grid, bad_grid = (C.c_float * 4)(0.0, 0.25, 0.5, 1.0), (C.c_float * 4)(0.0, float("inf"), 0.5, 1.0)
    good, bad = (C.c_float * 6)(1.5, 5.5, 1.5, 5.5, 1.5, 5.5), (C.c_float * 6)(1.5, 5.5, 1.5, float("nan"), 1.5, 5.5)
    who = "lt_sample_flowedit:"

    def call(*, zz=P(x), xs=P(x), nz=P(noise), g=grid, sc=good, ng=4, batch=4, h=16, ch=3, io=_lib.LT_BF16):
        a = eng._step_args(x, 1.0, 1.0, 1.0, None, False, cfg_channels=ch)
        a.batch, a.latent_h, a.io_dtype = batch, h, io
        return L.lt_sample_flowedit(eng.handle, zz, xs, nz, P(out), P(out[4 * n:]), g, sc, ng, C.byref(a), stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    null = C.c_void_p(0)
    for k in ("zz", "xs", "nz"):
        refused(call(**{k: null}), who, "null argument")
    refused(call(g=None), who, "null argument")
    refused(call(sc=None), who, "null argument")
    refused(call(ng=1), who, "2 grid points")
    for b in (6, 0, -4, 3):
        refused(call(batch=b), who, "multiple of 4")
    refused(call(batch=12), who, "outside 1..max_batch")
    refused(call(batch=8), who, "lt_prepare_prompt was called for batch 4, step has batch 8")
    refused(call(h=15), who, "multiple of the patch size")
    refused(call(io=_lib.LT_F16), "io_dtype")
    refused(call(ch=0), who, "cfg_channels 0")
    refused(call(ch=5), who, "cfg_channels 5")
    refused(call(sc=bad), who, "target scale of interval 1", "not finite")
    refused(call(g=bad_grid), who, "grid value 1", "not finite")
    # a stream under capture: refused before anything is launched, the caller's capture stays valid and its other content replays
    a = torch.arange(64, dtype=torch.float32, device="cuda")
    graph, side, seen = torch.cuda.CUDAGraph(), torch.cuda.Stream(), []
    with torch.cuda.graph(graph, stream=side):
        seen.append((call(), L.lt_last_error().decode()))
        b = a + 1.0
    rc, msg = seen[0]
    assert rc != 0 and who in msg and "capture" in msg, (rc, msg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(b, a + 1.0) and bool(torch.isnan(out).all())
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    eng.prepare_prompt_regional(cap, cmask, cap[:1].contiguous(), cmask[:1].contiguous(), 1, 1)
    refused(call(), who, "regional prompt")
    # the Python layer
    with pytest.raises(_lib.LuminaLibError, match="noise must be"):
        eng.sample_flowedit(x, [0.0, 0.5, 1.0], noise, E.flowedit_scales(2, 1.5, 5.5))
    with pytest.raises(_lib.LuminaLibError, match="2 grid points"):
        eng.sample_flowedit(x, [0.0], noise[:0], torch.zeros(0, 2))
    with pytest.raises(ValueError, match="multiple of 4"):
        model.sample_flowedit(x, [0.0, 0.5, 1.0], noise[:2], cap, cmask)
    with pytest.raises(TypeError, match="conditioning"):
        model.sample_flowedit(x, [0.0, 0.5, 1.0], noise[:2], feats, masks, feats)
    # ... and the same arguments untouched are served; the model call goes on as before
    eng.prepare_prompt(feats, masks)
    assert call() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert eng.last_nfe() == 3 and eng.last_eval_rows() == 12
    assert torch.equal(out[3 * n:4 * n].view_as(x), ref) and torch.equal(out[4 * n:].view_as(x), ref) and torch.equal(out[:n].view_as(x), x)
    assert torch.equal(model.sample_flowedit(x, [0.0, 0.25, 0.5, 1.0], noise, feats, masks, src_cfg=1.5, tgt_cfg=5.5), ref)


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_driver_makes_one_flowedit_call_and_with_n_min_one_more_ode_call(golden_dir, tmp_path, monkeypatch):
    from safetensors.torch import save_file

    from lumina_t2x_amd import sample_edit as S

    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_edit_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_edit_test"] = ctor
    (tmp_path / "targets.txt").write_text("a red cube\n")
    gen = torch.Generator().manual_seed(3)
    table = {c: torch.randn(16, cfg.cap_feat_dim, generator=gen) for c in ("a cube", "a red cube", "")}

    def encode(caps):
        feats = torch.stack([table[c] for c in caps]).to("cuda", torch.bfloat16)
        mask = torch.ones(len(caps), 16, dtype=torch.int64, device="cuda")
        mask[-2:, 8:] = 0
        return feats, mask

    decoded = []

    def decode(lat):
        decoded.append(lat.clone())
        return torch.sigmoid(lat[:, :3].float())

    img = (torch.rand(3, 128, 128, generator=gen) * 2 - 1).cuda()
    venc = lambda im: torch.nn.functional.avg_pool2d(im, 8)[:, [0, 1, 2, 0]]  # noqa: E731
    calls = []
    for name in ("sample_flowedit", "sample_ode"):
        def counted(self, *a, _name=name, _fn=getattr(DiTEngine, name), **k):
            calls.append(_name)
            return _fn(self, *a, **k)
        monkeypatch.setattr(DiTEngine, name, counted)
    argv = ["--ckpt", str(ck), "--image", "unused.png", "--source_caption", "a cube", "--caption_path", str(tmp_path / "targets.txt"),
            "--resolution", "256:128x128", "--num_sampling_steps", "8", "--time_shifting_factor", "4", "--strength", "0.75", "--seed", "11"]
    counts = {}
    try:
        for name, extra in (("plain", []), ("tail", ["--n_min", "2"])):
            del calls[:]
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, vae_encode_fn=venc, decode_fn=decode, image=img)
            counts[name] = (list(calls), built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
    finally:
        del models.__dict__["NextDiT_tiny_edit_test"]
    # 8 steps cut at strength 0.75: 6 grid points, 5 intervals; with --n_min 2 the edit takes 3 and lt_sample_ode the last 2 (2 rows each)
    assert counts == {"plain": (["sample_flowedit"], 5, 20), "tail": (["sample_flowedit", "sample_ode"], 2, 4)}
    rec = json.loads((tmp_path / "tail" / "data.json").read_text())[0]
    assert (rec["src_cfg"], rec["tgt_cfg"], rec["strength"], rec["n_min"], rec["seed"], rec["intervals"]) == (1.5, 5.5, 0.75, 2, 11, 5)
    model = built[0]
    grid = ODE(8, "euler", 4.0, strength=0.75).t
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    torch.random.manual_seed(11)
    x_src = (venc(img[None]) * 0.13025).to(torch.bfloat16)
    noise = torch.randn([5, 1, 4, 16, 16], device="cuda").to(torch.bfloat16)
    feats, mask = encode(["a cube", "a red cube", "", ""])
    want = model.sample_flowedit(x_src, grid, noise, feats, mask, src_cfg=1.5, tgt_cfg=5.5, **kw)
    assert torch.equal(decoded[0], want / 0.13025) and not torch.equal(want, x_src)
    torch.random.manual_seed(11)
    noise = torch.randn([3, 1, 4, 16, 16], device="cuda").to(torch.bfloat16)
    z = model.sample_flowedit(x_src, grid[:4], noise, feats, mask, src_cfg=1.5, tgt_cfg=5.5, **kw)
    start = E.edit_tail_start(z, x_src, torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16), float(grid[3]))
    tail = ODE(8, "euler", 4.0)
    tail.t = grid[3:]
    want = tail.sample(start.repeat(2, 1, 1, 1), model.forward_with_cfg, cap_feats=feats[[1, 3]].contiguous(), cap_mask=mask[[1, 3]].contiguous(),
                       cfg_scale=5.5, **kw)[-1][:1]
    assert torch.equal(decoded[1], want / 0.13025) and not torch.equal(decoded[1], decoded[0])
