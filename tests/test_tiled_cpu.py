"""CPU: tiled (MultiDiffusion) sampling - transport/tiled.py, the definition lt_forward_tiled / lt_sample_ode_tiled are held to.  No GPU.

* window_grid: the offsets as specified, covering, the last one clamped, every invalid combination refused;
* window_weights: strictly positive, symmetric, the float64 formula rounded once;
* fuse equals its float64 restatement word for word on operands where the sums are exact (tests/exact_tiled.py), on three geometries;
* sample_tiled: one window that is the canvas is the fixed-grid host loop, disjoint windows are the per-crop loops, bit for bit;
* the comparison can fail: a changed window order, a dropped division, a fused multiply-add each move a word;
* the C entries refuse by name without a device; the Python front ends refuse the combinations the call does not serve."""
import ctypes as C
import math
import types

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import tiled as T
from lumina_t2x_amd.transport.integrators import fixed_grid_odeint
from lumina_t2x_amd.transport.mini import ODE

import exact_tiled as X

DTYPES = [torch.bfloat16, torch.float32]
METHODS = ["euler", "midpoint", "rk4"]


# ---- window_grid ----------------------------------------------------------------------------------------------------------------------
def test_window_grid_offsets_are_as_specified():
    assert T.window_grid(8, 8, 8, 8, 4, 4) == [(0, 0)]
    assert T.window_grid(8, 12, 8, 8, 4, 4) == [(0, 0), (0, 4)]
    assert T.window_grid(12, 12, 8, 8, 4, 4) == [(0, 0), (0, 4), (4, 0), (4, 4)]
    assert T.window_grid(8, 14, 8, 8, 4, 4) == [(0, 0), (0, 4), (0, 6)]          # 8 would leave the canvas: clamped to 14 - 8
    assert T.window_grid(8, 16, 8, 8, 8, 8) == [(0, 0), (0, 8)]                  # disjoint
    assert T.window_grid(16, 48, 16, 16, 8, 8) == [(0, l) for l in (0, 8, 16, 24, 32)]
    assert T.window_grid(9, 9, 6, 6, 3, 3, patch_size=3) == [(0, 0), (0, 3), (3, 0), (3, 3)]


@pytest.mark.parametrize("canvas,win,stride", [((8, 14), (8, 8), (4, 4)), ((20, 26), (8, 12), (6, 10)), ((12, 12), (8, 8), (4, 4)),
                                               ((10, 10), (10, 4), (2, 2))])
def test_window_grid_covers_and_stays_inside(canvas, win, stride):
    offs = T.window_grid(*canvas, *win, *stride)
    assert offs == sorted(offs) and len(set(offs)) == len(offs)
    assert all(0 <= t <= canvas[0] - win[0] and 0 <= l <= canvas[1] - win[1] and t % 2 == 0 and l % 2 == 0 for t, l in offs)
    assert offs[-1] == (canvas[0] - win[0], canvas[1] - win[1])
    assert int(X.cover_counts(offs, win, canvas).min()) >= 1
    assert T.check_windows(offs, win, canvas) == offs


@pytest.mark.parametrize("args,needle", [
    ((8, 8, 10, 8, 4, 4), "larger than the canvas"), ((8, 8, 8, 10, 4, 4), "larger than the canvas"),
    ((16, 16, 8, 8, 10, 4), "leaves gaps"), ((16, 16, 8, 8, 4, 10), "leaves gaps"),
    ((9, 8, 8, 8, 4, 4), "multiple of the patch"), ((8, 8, 6, 7, 2, 2), "multiple of the patch"), ((8, 8, 8, 8, 3, 4), "multiple of the patch"),
    ((8, 8, 8, 8, 0, 4), "positive integer"), ((8, 8, 0, 8, 4, 4), "positive integer"), ((-8, 8, 8, 8, 4, 4), "positive integer"),
    ((8, 8, 8.0, 8, 4, 4), "positive integer"), ((8, 8, 8, 8, 4, True), "positive integer")])
def test_window_grid_refuses_invalid_combinations(args, needle):
    with pytest.raises(ValueError, match=needle):
        T.window_grid(*args)


def test_check_windows_refuses_tables_outside_the_canvas():
    for offs, needle in (([(0, 8)], "outside the canvas"), ([(-2, 0)], "outside the canvas"), ([], "1 .. 64 windows"),
                         ([(0, 0)] * 65, "1 .. 64 windows")):
        with pytest.raises(ValueError, match=needle):
            T.check_windows(offs, (8, 8), (8, 12))
    with pytest.raises(ValueError, match="does not fit"):
        T.check_windows([(0, 0)], (16, 8), (8, 12))
    with pytest.raises(ValueError, match="fp32 tensor"):
        T.check_windows([(0, 0)], (8, 8), (8, 12), torch.ones(8, 8, dtype=torch.float64))


# ---- window_weights -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(8, 8), (6, 10), (2, 2), (16, 4)])
def test_window_weights(h, w):
    u = T.window_weights(h, w)
    assert u.dtype == torch.float32 and torch.equal(u, torch.ones(h, w))
    c = T.window_weights(h, w, "cosine")
    assert c.dtype == torch.float32 and tuple(c.shape) == (h, w)
    assert float(c.min()) > 0 and bool(torch.isfinite(c).all())
    assert torch.equal(c, c.flip(0)) and torch.equal(c, c.flip(1))
    want = torch.tensor([[0.5 * (1 - math.cos(2 * math.pi * (i + 0.5) / h)) * (0.5 * (1 - math.cos(2 * math.pi * (j + 0.5) / w)))
                          for j in range(w)] for i in range(h)], dtype=torch.float64)
    # (math.cos and torch.cos may differ in the last float64 bit: one fp32 ulp at most where the product sits on a rounding boundary)
    assert torch.equal(c, torch.outer(*[0.5 * (1.0 - torch.cos(2.0 * math.pi * (torch.arange(n, dtype=torch.float64) + 0.5) / n))
                                        for n in (h, w)]).float())
    assert float((c.double() - want).abs().max()) <= 2.0 ** -24
    with pytest.raises(ValueError, match="not in"):
        T.window_weights(h, w, "hann")


# ---- fuse -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("geo", sorted(X.GEOMETRIES))
def test_fuse_equals_its_float64_restatement(geo, dtype):
    canvas, win, offs, weight = X.GEOMETRIES[geo]
    f = X.exact_f(len(offs), 3, *win, dtype, seed=11)
    got = T.fuse(f, offs, weight, canvas, dtype)
    assert got.dtype == dtype and tuple(got.shape) == (3,) + canvas
    assert torch.equal(X.words(got), X.words(X.fuse64(f, offs, weight, canvas, dtype)))
    cnt = X.cover_counts(offs, win, canvas)
    assert {"two_overlap": {1, 2}, "four_12x12": {1, 2, 4}, "clamped_8x14": {1, 2, 3}}[geo] == set(cnt.unique().tolist())
    # a pixel under one window is that window's value (the weight cancels exactly: it is a power of two)
    t, l = offs[0]
    only = cnt[t:t + win[0], l:l + win[1]] == 1
    assert torch.equal(got[:, t:t + win[0], l:l + win[1]][:, only], f[0][:, only])
    assert torch.equal(T.cover(offs, weight, canvas), sum(torch.nn.functional.pad(weight, (l, canvas[1] - l - win[1], t, canvas[0] - t - win[0]))
                                                          for t, l in offs))


@pytest.mark.parametrize("mutation", ["order", "nodiv", "fma"])
def test_the_comparison_can_fail(mutation):
    """random operands and cosine weights on the geometry with pixels under four windows, fp32 (a bf16 result may round a last-bit change
    away): each mutant of fuse moves at least one word, and the unmutated restatement moves none"""
    canvas, win, offs, _ = X.GEOMETRIES["four_12x12"]
    weight = T.window_weights(*win, "cosine")
    f = X.random_f(len(offs), 3, *win, torch.float32, seed=5)
    good = T.fuse(f, offs, weight, canvas, torch.float32)
    assert torch.equal(X.words(good), X.words(X.fuse_mutant(f, offs, weight, canvas, torch.float32, None)))
    moved = int((X.words(good) != X.words(X.fuse_mutant(f, offs, weight, canvas, torch.float32, mutation))).sum())
    assert moved >= 1, mutation


# ---- sample_tiled ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", METHODS)
def test_one_window_that_is_the_canvas_is_the_fixed_grid_loop(method, dtype):
    torch.manual_seed(3)
    z = torch.randn(1, 3, 8, 12).to(dtype)
    tgrid = torch.linspace(0, 1, 5) ** 2
    model = X.toy_model([0.7, 1.3])
    got = T.sample_tiled(model, z, tgrid, [(0, 0)], (8, 12), None, method)

    def plain(tt, y):
        return model(torch.cat([y, y]), torch.ones(2) * tt)[:1]

    want = fixed_grid_odeint(plain, z, tgrid, method=method)
    assert tuple(got.shape) == (5, 1, 3, 8, 12) and got.dtype == dtype
    assert torch.equal(X.words(got), X.words(want))
    v = T.tiled_velocity(model, z, torch.full((2,), 0.25), [(0, 0)], (8, 12), torch.ones(8, 12))
    assert torch.equal(X.words(v), X.words(model(torch.cat([z, z]), torch.full((2,), 0.25))[:1]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", METHODS)
def test_disjoint_windows_are_the_per_crop_loops(method, dtype):
    torch.manual_seed(4)
    z = torch.randn(1, 3, 8, 16).to(dtype)
    tgrid = torch.linspace(0, 1, 4)
    scales = [0.5, 1.5, 0.9, 1.1]  # rows 0, 1: the two windows' prompts; rows 2, 3: the negative prompts
    offs = T.window_grid(8, 16, 8, 8, 8, 8)
    got = T.sample_tiled(X.toy_model(scales), z, tgrid, offs, (8, 8), T.window_weights(8, 8, "cosine"), method)
    for k, (t, l) in enumerate(offs):
        one = X.toy_model([scales[k], scales[2 + k]])
        want = fixed_grid_odeint(lambda tt, y: one(torch.cat([y, y]), torch.ones(2) * tt)[:1], z[:, :, t:t + 8, l:l + 8].contiguous(), tgrid,
                                 method=method)
        if dtype == torch.float32:  # (w * f) / w is f only where the product is exact: compare against the same division
            w = T.window_weights(8, 8, "cosine")
            one_w = lambda tt, y: ((w * one(torch.cat([y, y]), torch.ones(2) * tt)[:1]) / w)  # noqa: E731
            want = fixed_grid_odeint(one_w, z[:, :, t:t + 8, l:l + 8].contiguous(), tgrid, method=method)
            assert torch.equal(X.words(got[:, :, :, t:t + 8, l:l + 8]), X.words(want))
    # with weight one the fusion is the identity at either dtype: the per-crop loops word for word
    got1 = T.sample_tiled(X.toy_model(scales), z, tgrid, offs, (8, 8), None, method)
    for k, (t, l) in enumerate(offs):
        one = X.toy_model([scales[k], scales[2 + k]])
        want = fixed_grid_odeint(lambda tt, y: one(torch.cat([y, y]), torch.ones(2) * tt)[:1], z[:, :, t:t + 8, l:l + 8].contiguous(), tgrid,
                                 method=method)
        assert torch.equal(X.words(got1[:, :, :, t:t + 8, l:l + 8]), X.words(want))


def test_sample_tiled_refuses_by_name():
    z = torch.zeros(1, 3, 8, 12)
    m = X.toy_model([1.0, 1.0])
    with pytest.raises(ValueError, match="fixed-grid methods"):
        T.sample_tiled(m, z, [0.0, 1.0], [(0, 0)], (8, 12), None, "dopri5")
    with pytest.raises(ValueError, match="ONE canvas latent"):
        T.sample_tiled(m, z.repeat(2, 1, 1, 1), [0.0, 1.0], [(0, 0)], (8, 12), None, "euler")
    with pytest.raises(ValueError, match="at least 2 grid points"):
        T.sample_tiled(m, z, [0.0], [(0, 0)], (8, 12), None, "euler")
    with pytest.raises(ValueError, match="outside the canvas"):
        T.sample_tiled(m, z, [0.0, 1.0], [(0, 8)], (8, 8), None, "euler")


# ---- the front ends -------------------------------------------------------------------------------------------------------------------
def test_ode_sample_routes_windows_and_refuses_combinations():
    torch.manual_seed(6)
    z = torch.randn(1, 3, 8, 12)
    offs = T.window_grid(8, 12, 8, 8, 4, 4)
    model = X.toy_model([0.5, 1.5, 0.9, 1.1])
    solver = ODE(4, "midpoint")
    got = solver.sample(z, model, windows=(offs, (8, 8)), window_weights=T.window_weights(8, 8, "cosine"))
    assert torch.equal(got, T.sample_tiled(model, z, solver.t, offs, (8, 8), T.window_weights(8, 8, "cosine"), "midpoint"))
    # without windows the call is the function it was
    assert torch.equal(solver.sample(z, X.toy_model([1.0])), fixed_grid_odeint(lambda tt, y: X.toy_model([1.0])(y, torch.ones(1) * tt), z, solver.t,
                                                                               method="midpoint"))
    win = dict(windows=(offs, (8, 8)))
    for extra, needle in ((dict(cfg_table=[1.0] * 6), "guidance table"), (dict(cfg_rescale=0.5), "rescale / norm limit"),
                          (dict(cfg_norm_limit=2.0), "rescale / norm limit"), (dict(cfg_reuse=[0] * 6), "guidance reuse"),
                          (dict(slg_table=[0.0] * 6), "skip-layer"), (dict(pag_table=[0.0] * 6), "perturbed-attention"),
                          (dict(cfg_apg=dict(eta=0.0, momentum=0.0, norm_threshold=1.0)), "projected"), (dict(cfg_zero_star=True), "projected"),
                          (dict(teacache=0.1), "step caching"), (dict(mask=torch.ones(8, 12)), "inpainting mask")):
        with pytest.raises(NotImplementedError, match=needle):
            solver.sample(z, model, **win, **extra)
    with pytest.raises(NotImplementedError, match="packed batch"):
        solver.sample([z[0]], model, **win)
    for method in ("ab2", "abm3", "dopri5"):
        with pytest.raises(NotImplementedError, match="multistep and adaptive"):
            ODE(4, method).sample(z, model, **win)
    with pytest.raises(ValueError, match="belongs to tiled sampling"):
        solver.sample(z, model, window_weights=torch.ones(8, 8))
    with pytest.raises(ValueError, match="windows must be"):
        solver.sample(z, model, windows=(offs,))


def test_sampler_sample_ode_routes_windows():
    from lumina_t2x_amd.transport import Sampler, create_transport
    torch.manual_seed(7)
    z = torch.randn(1, 3, 8, 12)
    offs = T.window_grid(8, 12, 8, 8, 4, 4)
    model = X.toy_model([0.5, 1.5, 0.9, 1.1])
    fn = Sampler(create_transport("Linear", "velocity", None, None, None)).sample_ode(sampling_method="euler", num_steps=3)
    got = fn(z, model, windows=(offs, (8, 8)))
    assert torch.equal(got, T.sample_tiled(model, z, fn.__self__.t, offs, (8, 8), None, "euler"))
    with pytest.raises(NotImplementedError, match="guidance table"):
        fn(z, model, windows=(offs, (8, 8)), cfg_table=[1.0, 1.0])


def test_driver_tile_arguments():
    from lumina_t2x_amd import sample as S
    args = S.build_parser().parse_args(["--ckpt", "x", "--tile", "64", "128"]) if hasattr(S, "build_parser") else None
    ns = types.SimpleNamespace(tile=(64, 128), tile_stride=None, tile_weights="cosine")
    (offs, win), w = S.tile_windows(ns, (32, 8), 2)  # canvas latent [w / 8, h / 8] = [256 / 8, 64 / 8]
    assert win == (16, 8) and offs == T.window_grid(32, 8, 16, 8, 8, 4) and torch.equal(w, T.window_weights(16, 8, "cosine"))
    ns = types.SimpleNamespace(tile=(64, 128), tile_stride=(64, 32), tile_weights="uniform")
    (offs, win), w = S.tile_windows(ns, (32, 8), 2)
    assert offs == [(0, 0), (4, 0), (8, 0), (12, 0), (16, 0)] and torch.equal(w, torch.ones(16, 8))
    for bad in ((60, 128), (64, 8), (0, 64)):
        with pytest.raises(SystemExit, match="multiples of 16"):
            S.tile_windows(types.SimpleNamespace(tile=bad, tile_stride=None, tile_weights="uniform"), (32, 8), 2)
    assert args is None or tuple(args.tile) == (64, 128)


# ---- the C entries, without a device --------------------------------------------------------------------------------------------------
NEW = ("lt_set_windows", "lt_forward_tiled", "lt_sample_ode_tiled", "lt_op_windows_gather", "lt_op_windows_reduce", "lt_op_windows_cover")


def test_headers_declare_the_calls():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(lib, name), name


def test_argument_errors_come_back_by_name_without_a_device():
    lib = _lib.load()
    a = _lib.LtStepArgs(batch=2, io_dtype=_lib.LT_BF16, latent_h=8, latent_w=8)
    grid = (C.c_float * 2)(0.0, 1.0)
    one, null = C.c_void_p(64), C.c_void_p(0)  # never dereferenced: every call below is refused before it reads anything
    offs = (C.c_int32 * 4)(0, 0, 0, 4)
    assert lib.lt_set_windows(None, offs, 2, 8, 8, 8, 12, None, None) != 0 and b"lt_set_windows: null engine" in lib.lt_last_error()
    assert lib.lt_forward_tiled(None, one, one, one, C.byref(a), None) != 0 and b"lt_forward_tiled: null argument" in lib.lt_last_error()
    assert lib.lt_sample_ode_tiled(None, one, None, one, grid, 2, 0, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_tiled: null argument" in lib.lt_last_error()
    # the op entries check the table on the host before anything is launched
    for n, wh, ww, ch, cw, needle in ((0, 8, 8, 8, 12, b"0 windows"), (65, 8, 8, 8, 12, b"65 windows"), (2, 8, 8, 8, 10, b"outside the canvas"),
                                      (2, 16, 8, 8, 12, b"window <= canvas"), (2, 0, 8, 8, 12, b"window <= canvas")):
        big = (C.c_int32 * 130)(*([0, 0, 0, 4] + [0] * 126))
        assert lib.lt_op_windows_gather(one, big, n, wh, ww, ch, cw, one, 3, 1, None) != 0 and needle in lib.lt_last_error(), lib.lt_last_error()
        assert lib.lt_op_windows_reduce(one, big, n, wh, ww, ch, cw, None, one, one, 3, 1, None) != 0 and needle in lib.lt_last_error()
        assert lib.lt_op_windows_cover(big, n, wh, ww, ch, cw, None, one, one, None) != 0 and needle in lib.lt_last_error()
    assert lib.lt_op_windows_gather(one, None, 2, 8, 8, 8, 12, one, 3, 1, None) != 0 and b"lt_op_windows_gather: null argument" in lib.lt_last_error()
    assert lib.lt_op_windows_gather(null, offs, 2, 8, 8, 8, 12, one, 3, 1, None) != 0 and b"windows_gather: null argument" in lib.lt_last_error()
    assert lib.lt_op_windows_gather(one, offs, 2, 8, 8, 8, 12, one, 3, 7, None) != 0 and b"f32 or bf16" in lib.lt_last_error()
    assert lib.lt_op_windows_reduce(one, offs, 2, 8, 8, 8, 12, None, null, one, 3, 1, None) != 0 and b"windows_reduce: null argument" in lib.lt_last_error()
    assert lib.lt_op_windows_cover(offs, 2, 8, 8, 8, 12, None, one, null, None) != 0 and b"windows_cover: null argument" in lib.lt_last_error()
