"""-m gpu: tiled (MultiDiffusion) sampling inside the engine - lt_set_windows / lt_forward_tiled / lt_sample_ode_tiled.

The reference has no such sampler; the pin is the host loop of plain torch expressions (transport/tiled.py) around the same engine-backed model:

* the three op entries against torch slicing and ``fuse``, every output word compared as an integer, on operands where the fusion is exact
  and on random ones, at every group width the launchers choose (4, 2, 1 pixels), outputs pre-filled with NaN;
* lt_set_windows refuses by name and leaves the table in force as it was;
* one window that is the canvas is lt_sample_ode(use_cfg = 1); disjoint windows are lt_sample_ode on the batch of the crops - word for word
  after mapping -0 to +0: the fusion adds the prediction to +0, and (+0) + (-0) is +0;
* overlapping windows with a prompt each and cosine weights equal sample_tiled around model.forward_with_cfg at every trajectory slot, bit
  for bit, and lt_forward_tiled equals tiled_velocity; once with class labels;
* the evaluation counts; a plain lt_sample_ode is what it was before and after a tiled call; a tiled call without a table is refused by name;
* the sample driver with --tile produces model.sample_ode_tiled's output, and without it makes the calls it made."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import tiled as T
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

import exact_tiled as X
from gpu_util import P, lib, stream
from test_gpu_sde import _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
METHODS = ["euler", "midpoint", "rk4"]
OP_GEOMETRIES = dict(X.GEOMETRIES, **X.GPU_EXTRA)
OP_GEOMETRIES["odd_5x9"] = ((5, 9), (5, 5), [(0, 0), (0, 3), (0, 4)], torch.full((5, 5), 2.0))  # nothing divides: one pixel per thread
_CACHE = {}


def _offs(offs):
    return (C.c_int32 * (2 * len(offs)))(*[v for o in offs for v in o])


def _code(dtype):
    return _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("geo", sorted(OP_GEOMETRIES))
def test_op_entries_equal_slicing_and_fuse_word_for_word(geo, dtype):
    canvas, win, offs, w_exact = OP_GEOMETRIES[geo]
    n, Cc = len(offs), 3
    L, arr = lib(), _offs(offs)
    # gather: exact copies into rows 0 .. n-1, the second half of the 2 n rows untouched
    y = torch.randn(1, Cc, *canvas, generator=torch.Generator().manual_seed(2)).to("cuda", dtype)
    rows = torch.full((2 * n, Cc) + win, float("nan"), dtype=dtype, device="cuda")
    _lib.check(L.lt_op_windows_gather(P(y), arr, n, *win, *canvas, P(rows), Cc, _code(dtype), stream()), "lt_op_windows_gather")
    assert torch.equal(X.words(rows[:n]), X.words(T.crop(y.cpu(), offs, win)))
    assert bool(torch.isnan(rows[n:].float()).all())
    for kind, weight in (("exact", w_exact), ("random", T.window_weights(*win, "cosine"))):
        f = (X.exact_f if kind == "exact" else X.random_f)(n, Cc, *win, dtype, seed=7)
        wd = weight.cuda()
        wsum = torch.full((canvas[0] * canvas[1] + 16,), float("nan"), device="cuda")
        bad = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        _lib.check(L.lt_op_windows_cover(arr, n, *win, *canvas, P(wd), P(wsum), P(bad), stream()), "lt_op_windows_cover")
        assert int(bad) == 0 and bool(torch.isnan(wsum[canvas[0] * canvas[1]:]).all())
        assert torch.equal(X.words(wsum[:canvas[0] * canvas[1]].view(canvas)), X.words(T.cover(offs, weight, canvas)))
        out = torch.full((Cc * canvas[0] * canvas[1] + 16,), float("nan"), dtype=dtype, device="cuda")
        _lib.check(L.lt_op_windows_reduce(P(f.cuda()), arr, n, *win, *canvas, P(wd), P(wsum), P(out), Cc, _code(dtype), stream()),
                   "lt_op_windows_reduce")
        want = T.fuse(f, offs, weight, canvas, dtype)
        got = out[:want.numel()].view(want.shape)
        diff = X.words(got) != X.words(want)
        assert not bool(diff.any()), (geo, kind, int(diff.sum()))
        assert bool(torch.isnan(out[want.numel():].float()).all())
        if kind == "exact":
            assert torch.equal(X.words(want), X.words(X.fuse64(f, offs, weight, canvas, dtype)))
    # null weights are ones
    ones = torch.ones(win)
    f = X.random_f(n, Cc, *win, dtype, seed=8)
    wsum = torch.empty(canvas[0] * canvas[1], device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L.lt_op_windows_cover(arr, n, *win, *canvas, None, P(wsum), P(bad), stream()), "lt_op_windows_cover")
    out = torch.empty((Cc,) + canvas, dtype=dtype, device="cuda")
    _lib.check(L.lt_op_windows_reduce(P(f.cuda()), arr, n, *win, *canvas, None, P(wsum), P(out), Cc, _code(dtype), stream()), "lt_op_windows_reduce")
    assert torch.equal(X.words(out), X.words(T.fuse(f, offs, ones, canvas, dtype)))


def test_cover_counts_the_uncovered_pixels_of_a_table_with_a_hole():
    offs, win, canvas = [(0, 0), (0, 8)], (8, 8), (8, 20)  # columns 16 .. 19 lie under no window
    wsum = torch.empty(canvas[0] * canvas[1], device="cuda")
    bad = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib().lt_op_windows_cover(_offs(offs), 2, *win, *canvas, None, P(wsum), P(bad), stream()), "lt_op_windows_cover")
    cnt = X.cover_counts(offs, win, canvas)
    assert int(bad) == int((cnt == 0).sum()) == 32
    assert torch.equal(wsum.cpu().view(canvas), cnt.float())
    # a weight that is not above 0 counts too
    w = torch.ones(win)
    w[0, 0] = 0.0
    _lib.check(lib().lt_op_windows_cover(_offs(offs), 2, *win, *canvas, P(w.cuda()), P(wsum), P(bad), stream()), "lt_op_windows_cover")
    assert int(bad) == 34


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
def _next(golden_dir, name="nextdit_tiny", rows=4):
    """the tiny text model and ``rows`` prompt rows (the window prompts, then the negative prompts)"""
    if name not in _CACHE:
        g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
        cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
        m = models.NextDiT(**cfg.ctor_kwargs())
        m.load_state_dict(synth.synth_state_dict(cfg, seed=int(g["seed_w"])), strict=True)
        _CACHE[name] = (m.eval().to("cuda", torch.bfloat16), cfg)
    m, cfg = _CACHE[name]
    gen = torch.Generator().manual_seed(17)
    cap = torch.randn(rows, 12, cfg.cap_feat_dim, generator=gen).to("cuda", torch.bfloat16)
    mask = torch.ones(rows, 12, dtype=torch.int64, device="cuda")
    mask[rows // 2:, 6:] = 0
    return m, cap, mask


STEP = dict(proportional_attn=True, base_seqlen=16)


def _tgrid(method):
    return ODE(4, method, 4).t


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", METHODS)
def test_one_window_that_is_the_canvas_is_lt_sample_ode(golden_dir, method, dtype):
    model, cap, mask = _next(golden_dir, rows=2)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(1)).to("cuda", dtype)
    tgrid = _tgrid(method)
    got = model.sample_ode_tiled(z, tgrid, ([(0, 0)], (16, 16)), cap, mask, 4.0, method=method, return_trajectory=True, **STEP)
    eng = model._engine
    stages = {"euler": 1, "midpoint": 2, "rk4": 4}[method]
    assert eng.last_nfe() == 3 * stages and eng.last_eval_rows() == 2 * 3 * stages
    want = model._engine_sample_ode(z.repeat(2, 1, 1, 1), tgrid, method, True, True, dict(cap_feats=cap, cap_mask=mask, cfg_scale=4.0, **STEP))
    assert tuple(got.shape) == (4, 1, 4, 16, 16) and got.dtype == dtype and bool(torch.isfinite(want.float()).all())
    # compared as integers after mapping -0 to +0: the fusion adds the prediction to +0, which turns a -0 into +0
    assert torch.equal(X.words(got), X.words(want[:, :1]))
    assert torch.equal(model.sample_ode_tiled(z, tgrid, ([(0, 0)], (16, 16)), cap, mask, 4.0, method=method, **STEP), got[-1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_disjoint_windows_are_lt_sample_ode_on_the_crops(golden_dir, dtype):
    model, cap, mask = _next(golden_dir, rows=4)
    z = torch.randn(1, 4, 8, 16, generator=torch.Generator().manual_seed(2)).to("cuda", dtype)
    offs = T.window_grid(8, 16, 8, 8, 8, 8)
    assert offs == [(0, 0), (0, 8)]
    for method in METHODS:
        tgrid = _tgrid(method)
        got = model.sample_ode_tiled(z, tgrid, (offs, (8, 8)), cap, mask, 4.0, method=method, return_trajectory=True, **STEP)
        crops = T.crop(z, offs, (8, 8))
        want = model._engine_sample_ode(torch.cat([crops, crops]).contiguous(), tgrid, method, True, True,
                                        dict(cap_feats=cap, cap_mask=mask, cfg_scale=4.0, **STEP))
        for k, (t, l) in enumerate(offs):
            assert torch.equal(X.words(got[:, 0, :, t:t + 8, l:l + 8]), X.words(want[:, k])), (method, k)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("name,canvas,win,stride", [("nextdit_tiny", (16, 24), (16, 16), (8, 8)), ("nextdit_tiny_rect", (12, 28), (12, 20), (8, 8)),
                                                    ("nextdit_tiny", (10, 10), (8, 8), (4, 4))])  # (0 | 2, 0 | 2): both last offsets clamped
def test_overlapping_windows_equal_the_host_loop_bit_for_bit(golden_dir, name, canvas, win, stride, dtype):
    offs = T.window_grid(*canvas, *win, *stride)
    n = len(offs)
    assert n in (2, 4) and int(X.cover_counts(offs, win, canvas).max()) >= 2
    model, cap, mask = _next(golden_dir, name, rows=2 * n)
    weight = T.window_weights(*win, "cosine")
    z = torch.randn(1, 4, *canvas, generator=torch.Generator().manual_seed(3)).to("cuda", dtype)
    kw = dict(cap_feats=cap, cap_mask=mask, cfg_scale=4.0, **STEP)
    t = torch.full((2 * n,), 0.3, device="cuda")
    v = model.forward_with_cfg_tiled(z, t, (offs, win), cap, mask, 4.0, weights=weight, **STEP)
    want_v = T.tiled_velocity(model.forward_with_cfg, z, t, offs, win, weight, **kw)
    assert bool(torch.isfinite(want_v.float()).all()) and torch.equal(v, want_v)
    for method in METHODS if name == "nextdit_tiny" and n == 2 else ["midpoint"]:
        tgrid = _tgrid(method)
        got = model.sample_ode_tiled(z, tgrid, (offs, win), cap, mask, 4.0, method=method, weights=weight, return_trajectory=True, **STEP)
        want = T.sample_tiled(model.forward_with_cfg, z, tgrid, offs, win, weight, method, **kw)
        assert got.shape == want.shape == (4, 1, 4) + canvas and got.dtype == dtype
        for i in range(4):
            assert torch.equal(got[i], want[i]), (method, i, int((got[i] != want[i]).sum()))
        # through the transport front end: the same call, and the host loop with use_engine = False
        o = ODE(4, method, 4)
        assert torch.equal(o.sample(z, model.forward_with_cfg, windows=(offs, win), window_weights=weight, **kw), got)
        o.use_engine = False
        assert torch.equal(o.sample(z, model.forward_with_cfg, windows=(offs, win), window_weights=weight, **kw), got)
    # the prompts matter: with the two windows' prompts swapped the canvas differs
    perm = list(reversed(range(n))) + list(range(n, 2 * n))
    assert not torch.equal(model.forward_with_cfg_tiled(z, t, (offs, win), cap[perm], mask[perm], 4.0, weights=weight, **STEP), v)


def test_class_labels_equal_the_host_loop(golden_dir):
    model, _, kw = _model(golden_dir, "imagenet")
    offs, win, canvas = [(0, 0), (0, 8)], (16, 16), (16, 24)
    y = torch.tensor([3, 7, 10, 10], device="cuda")
    weight = T.window_weights(*win, "cosine")
    z = torch.randn(1, 4, *canvas, generator=torch.Generator().manual_seed(5)).to("cuda", torch.bfloat16)
    tgrid = _tgrid("midpoint")
    got = model.sample_ode_tiled(z, tgrid, (offs, win), y, 4.0, method="midpoint", weights=weight, return_trajectory=True)
    want = T.sample_tiled(model.forward_with_cfg, z, tgrid, offs, win, weight, "midpoint", y=y, cfg_scale=4.0)
    assert bool(torch.isfinite(want.float()).all()) and torch.equal(got, want)
    t = torch.full((4,), 0.6, device="cuda")
    assert torch.equal(model.forward_with_cfg_tiled(z, t, (offs, win), y, 4.0, weights=weight),
                       T.tiled_velocity(model.forward_with_cfg, z, t, offs, win, weight, y=y, cfg_scale=4.0))


def test_counts_and_the_plain_call_around_a_tiled_call(golden_dir):
    model, cap, mask = _next(golden_dir, rows=4)
    offs, win = [(0, 0), (0, 8)], (16, 16)
    z = torch.randn(1, 4, 16, 24, generator=torch.Generator().manual_seed(6)).to("cuda", torch.bfloat16)
    zp = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(7)).to("cuda", torch.bfloat16)
    tgrid = _tgrid("rk4")
    pkw = dict(cap_feats=cap[:2], cap_mask=mask[:2], cfg_scale=4.0, **STEP)
    model.sample_ode_tiled(z, tgrid[:2], (offs, win), cap, mask, 4.0, method="euler", **STEP)  # (the engine of all three calls below exists)
    first = model._engine
    before = model._engine_sample_ode(zp, tgrid, "rk4", True, True, dict(pkw))
    model.sample_ode_tiled(z, tgrid, (offs, win), cap, mask, 4.0, method="rk4", **STEP)
    eng = model._engine
    assert eng.last_nfe() == 3 * 4 and eng.last_eval_rows() == 3 * 4 * 4
    after = model._engine_sample_ode(zp, tgrid, "rk4", True, True, dict(pkw))
    assert eng.last_nfe() == 12 and eng.last_eval_rows() == 24
    assert eng is first and torch.equal(X.words(before), X.words(after))
    # dropping the table: a tiled call is refused by name, the output untouched
    eng.prepare_prompt(cap, mask)
    key = eng._windows_key
    eng.set_windows(None, None, None)
    assert eng._windows_key is None
    with pytest.raises(_lib.LuminaLibError, match="no window table"):
        eng.sample_ode_tiled(z, tgrid, "euler")
    eng._windows_key = key  # (past the wrapper's own check: the C entry refuses)
    for call in (lambda: eng.sample_ode_tiled(z, tgrid, "euler"), lambda: eng.forward_tiled(z, torch.zeros(4, device="cuda"))):
        with pytest.raises(_lib.LuminaLibError, match=r"lt_(sample_ode|forward)_tiled: no window table \(call lt_set_windows first\)"):
            call()
    eng._windows_key = None
    eng._windows_src = (None,)


def test_set_windows_refuses_by_name_and_keeps_the_table_in_force(golden_dir):
    model, cap, mask = _next(golden_dir, rows=4)
    offs, win, canvas = [(0, 0), (0, 8)], (16, 16), (16, 24)
    weight = T.window_weights(*win, "cosine")
    z = torch.randn(1, 4, *canvas, generator=torch.Generator().manual_seed(8)).to("cuda", torch.bfloat16)
    t = torch.full((4,), 0.4, device="cuda")
    ref = model.forward_with_cfg_tiled(z, t, (offs, win), cap, mask, 4.0, weights=weight, **STEP)
    eng, L = model._engine, lib()
    mb = eng.limits.max_batch
    assert mb >= 4 and eng.limits.max_tokens >= 64
    s = stream()
    wd = weight.cuda()
    hole = torch.ones(16, 16, device="cuda")
    hole[3, 3] = float("inf")
    tok = eng.limits.max_tokens
    cases = [
        ((None, 2, 16, 16, 16, 24, None), "null argument"),
        ((_offs([(0, 0)] * 65), 65, 16, 16, 16, 24, None), r"n = 65 windows"),
        ((_offs(offs), -1, 16, 16, 16, 24, None), r"n = -1 windows"),
        ((_offs([(0, 0)] * (mb // 2 + 1)), mb // 2 + 1, 16, 16, 16, 24, None), rf"2 n = {2 * (mb // 2 + 1)} rows.*max_batch is {mb}"),
        ((_offs(offs), 2, 15, 16, 16, 24, None), "multiples of the patch size"),
        ((_offs(offs), 2, 16, 16, 16, 23, None), "multiples of the patch size"),
        ((_offs([(0, 0), (0, 7)]), 2, 16, 16, 16, 24, None), r"offset \(0, 7\) of window 1 is not a multiple"),
        ((_offs([(0, 0), (0, 10)]), 2, 16, 16, 16, 24, None), "outside the canvas"),
        ((_offs([(0, 0), (2, 0)]), 2, 16, 16, 16, 24, None), "outside the canvas"),
        ((_offs(offs), 2, 32, 16, 16, 24, None), "1 <= window <= canvas"),
        ((_offs([(0, 0), (0, 2)]), 2, 2 * tok, 4, 2 * tok, 6, None), rf"{2 * tok} latent tokens, max_tokens is {tok}"),
        ((_offs([(0, 0), (0, 0)]), 2, 16, 16, 16, 34, None), "cannot be covered by 2 windows"),
        ((_offs([(0, 0), (0, 0)]), 2, 16, 16, 16, 24, None), r"not covered: 128 of its 384 pixels"),
        ((_offs(offs), 2, 16, 16, 16, 24, C.c_void_p(hole.data_ptr())), r"not covered: \d+ of its 384 pixels"),
    ]
    for (arr, n, wh, ww, ch, cw, wp), needle in cases:
        rc = L.lt_set_windows(eng.handle, arr, n, wh, ww, ch, cw, wp, s)
        msg = L.lt_last_error().decode()
        assert rc != 0 and re.search(needle, msg), (needle, msg)
        assert msg.startswith("lt_set_windows: "), msg
    assert L.lt_set_windows(None, _offs(offs), 2, 16, 16, 16, 24, None, s) != 0 and b"lt_set_windows: null engine" in L.lt_last_error()
    # the table that was set is still the one in force, weights and sums included
    assert torch.equal(eng.forward_tiled(z, t, cfg_scale=4.0, **STEP), ref)
    # the call's own refusals, by name
    a = eng._tiled_args(z, "test", 4.0, 1.0, 1.0, 16, True, 1.0)
    out = torch.full_like(z, float("nan"))
    grid = (C.c_float * 2)(0.0, 1.0)

    def sample(args, method=0):
        return L.lt_sample_ode_tiled(eng.handle, P(z), None, P(out), grid, 2, method, 1, C.byref(args), s)

    for field, value, needle in (("batch", 2, r"a->batch = 2 n = 4"), ("latent_h", 8, r"windows of 16x16, the call has a latent of 8x16"),
                                 ("io_dtype", _lib.LT_F16, "io_dtype")):
        b = _lib.LtStepArgs.from_buffer_copy(a)
        setattr(b, field, value)
        assert sample(b) != 0 and re.search(needle, L.lt_last_error().decode()), L.lt_last_error()
        assert L.lt_forward_tiled(eng.handle, P(z), P(t), P(out), C.byref(b), s) != 0
        assert re.search(needle, L.lt_last_error().decode()), L.lt_last_error()
    assert sample(a, 7) != 0 and b"lt_sample_ode_tiled: unknown method 7" in L.lt_last_error()
    assert sample(a, _lib.LT_ODE_AB2) != 0 and b"unknown method" in L.lt_last_error()
    assert L.lt_sample_ode_tiled(eng.handle, P(z), None, P(out), grid, 1, 0, 1, C.byref(a), s) != 0 and b"at least 2 grid points" in L.lt_last_error()
    eng.prepare_prompt(cap[:2], mask[:2])
    assert sample(a) != 0 and b"lt_prepare_prompt was called for batch 2, 2 windows need 4 rows" in L.lt_last_error()
    eng.prepare_prompt(cap, mask)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all())
    # the Python wrappers refuse what the call does not serve, by name
    with pytest.raises(_lib.LuminaLibError, match="fixed-grid methods"):
        model.sample_ode_tiled(z, [0.0, 1.0], (offs, win), cap, mask, 4.0, method="ab2", **STEP)
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.sample_ode_tiled([z[0]], [0.0, 1.0], (offs, win), cap, mask, 4.0, **STEP)
    with pytest.raises(_lib.LuminaLibError, match="2 n = 4 rows of cap_feats"):
        model.sample_ode_tiled(z, [0.0, 1.0], (offs, win), cap[:3], mask[:3], 4.0, **STEP)
    with pytest.raises(_lib.LuminaLibError, match="outside the canvas"):
        model.sample_ode_tiled(z, [0.0, 1.0], ([(0, 0), (0, 10)], win), cap, mask, 4.0, **STEP)
    # one prompt and one negative prompt serve every window
    both = model.forward_with_cfg_tiled(z, t, (offs, win), cap[[0, 2]], mask[[0, 2]], 4.0, weights=weight, **STEP)
    assert torch.equal(both, model.forward_with_cfg_tiled(z, t, (offs, win), cap[[0, 0, 2, 2]], mask[[0, 0, 2, 2]], 4.0, weights=weight, **STEP))


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_sample_driver_with_tiles_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_tiled_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_tiled_test"] = ctor
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

    argv = ["--ckpt", str(ck), "--caption_path", str(tmp_path / "prompts.txt"), "--num_sampling_steps", "5", "--sampling-method", "midpoint",
            "--time_shifting_factor", "4", "--seed", "11"]
    runs = {}
    try:
        for name, extra in (("default", ["--resolution", "256:128x128"]),
                            ("tiled", ["--resolution", "256:128x192", "--tile", "128", "128", "--tile_weights", "cosine"])):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            runs[name] = (built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
        with pytest.raises(SystemExit, match="--tile is not served together"):
            S.run(S.build_parser().parse_args(argv + ["--resolution", "256:128x192", "--tile", "128", "128", "--cfg_interval", "0.1", "0.8",
                                                      "--image_save_path", str(tmp_path / "no")]),
                  encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
    finally:
        del models.__dict__["NextDiT_tiny_tiled_test"]
    # every evaluation of a run lies in ONE whole-trajectory call: 4 intervals x 2 stages, of 2 rows / of 2 n = 4 rows
    assert runs == {"default": (8, 16), "tiled": (8, 32)}
    fn = Sampler(create_transport()).sample_ode(sampling_method="midpoint", num_steps=5, time_shifting_factor=4.0)
    tgrid = fn.__self__.t
    feats, mask = encode(["a red cube", ""])
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    # without --tile the driver makes the call it made
    assert torch.equal(decoded[0], fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1] / 0.13025)
    torch.manual_seed(11)
    zc = torch.randn([1, 4, 16, 24], device="cuda").to(torch.bfloat16)
    offs = T.window_grid(16, 24, 16, 16, 8, 8)
    want = model.sample_ode_tiled(zc, tgrid, (offs, (16, 16)), feats, mask, 4.0, method="midpoint", weights=T.window_weights(16, 16, "cosine"), **kw)
    assert tuple(decoded[1].shape) == (1, 4, 16, 24) and torch.equal(decoded[1], want / 0.13025)
