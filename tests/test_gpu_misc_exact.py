"""-m gpu: the sixteen kernels of csrc/misc.hip and the stand-alone router of csrc/moe.hip through their op-level entries (lumina_dit_debug.h)
against the references of tests/exact_misc.py: movement and conversions as integer words, rounding chains word for word (both neighbours only where a
stage's float64 value lies within its bound of a bf16 midpoint, share capped), the fp32 ODE state bit for bit against numpy float32, the fp32 RoPE
table inside its derived bound.  Every output lies in a sentinel-filled buffer between guard zones; words a kernel must not write keep the sentinel.
Shapes are the smallest that reach each path; every grid-stride kernel has one case past launch cap x 256 elements (a second pass of its loop)."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_misc as M
import exact_rows as R
from exact_operands import int_bias
from gpu_util import P, lib, ok, stream

pytestmark = pytest.mark.gpu
DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


class Bufs:
    """device copies between guard zones, outputs pre-filled with the sentinel; done() synchronises and checks every guard"""

    def __init__(self):
        self.guards = []

    def put(self, t):
        if t is None:
            return None
        g, view = R.guarded_copy(t.contiguous())
        self.guards.append(g)
        return view

    def out(self, *shape, dtype=torch.bfloat16):
        g = M.guarded(int(np.prod(shape)), dtype=dtype)
        self.guards.append(g)
        return g.out.view(*shape)

    def done(self, what):
        torch.cuda.synchronize()
        for g in self.guards:
            g.assert_intact(what)


def _report(kernel, shape, share=0.0, bound="one word", dist=None):
    extra = "" if dist is None else f" worst_distance={dist:.3f}"
    print(f"EXACT kernel={kernel} shape={shape} ambiguous={share:.4%} bound={bound}{extra}")


# ---- a / b: movement and conversions ---------------------------------------------------------------------------------------------------------
# (x_dtype, B, C, H, W, patch, kpad, dup_first_half, eol)
PATCHIFY = [(1, 2, 4, 16, 16, 2, 16, 0, 0), (0, 2, 4, 16, 16, 2, 16, 0, 0), (1, 2, 4, 8, 24, 2, 32, 0, 0), (0, 2, 4, 8, 24, 2, 32, 1, 0),
            (1, 6, 4, 16, 16, 2, 32, 1, 0), (1, 2, 4, 8, 24, 2, 16, 0, 1), (0, 6, 4, 8, 24, 2, 32, 1, 1), (1, 1, 4, 16, 16, 2, 16, 0, 0),
            (0, 1, 4, 8, 24, 2, 32, 0, 1), (1, 2, 4, 368, 368, 2, 32, 0, 0), (0, 2, 4, 368, 368, 2, 32, 1, 0)]


@pytest.mark.parametrize("c", PATCHIFY, ids=lambda c: "-".join(map(str, c)))
def test_patchify_moves_and_converts_every_word(c):
    xd, B, Cc, H, W, p, kpad, dup, eol = c
    Hp, Wp = H // p, W // p
    wps = Wp + 1 if eol else 0
    x = M.source(xd, B * Cc * H * W, sum(c)).view(B, Cc, H, W)
    w, nan = M.convert_words(x)
    want = M.ref_patchify(w, p, kpad, dup, wps)
    nmask = None if nan is None else (M.ref_patchify(nan.astype(np.int16), p, kpad, dup, wps) == 1)
    b = Bufs()
    xg, out = b.put(x), b.out(*want.shape)
    what = f"patchify {c}"
    assert want.size > 8192 * 256 or H < 100
    ok(lib().lt_op_patchify(P(xg), xd, P(out), B, Cc, H, W, p, kpad, dup, wps, stream()), what)
    b.done(what)
    M.assert_bits(M.bits(out), want, what, nmask)
    _report("patchify_kernel", c)


@pytest.mark.parametrize("rows_total,Wp,d", [(3, 1, 64), (5, 8, 64), (3, 1, 2304), (5, 8, 2304), (4100, 1, 2304)], ids=str)
def test_eol_fill_writes_the_eol_rows_only(rows_total, Wp, d):
    x, eol = M.random_words((rows_total * (Wp + 1), d), d + Wp), M.random_words((d,), d + Wp + 1)
    want = M.ref_eol_fill(M.bits(x), M.bits(eol), rows_total, Wp)
    b = Bufs()
    xg, eg = b.put(x), b.put(eol)
    what = f"eol_fill rows {rows_total} Wp {Wp} d {d}"
    assert rows_total < 100 or rows_total * (d // 8) > 4096 * 256
    ok(lib().lt_op_eol_fill(P(xg), P(eg), rows_total, Wp, d, stream()), what)
    b.done(what)
    M.assert_bits(M.bits(xg), want, what)
    _report("eol_fill_kernel", (rows_total, Wp, d))


@pytest.mark.parametrize("rows,d", [(1, 8), (7, 8), (1, 2304), (7, 2304), (920, 2304)], ids=str)
def test_fill_rows_repeats_the_row(rows, d):
    row = M.random_words((d,), rows + d)
    b = Bufs()
    rg, out = b.put(row), b.out(rows, d)
    assert rows < 100 or rows * d > 8192 * 256
    ok(lib().lt_op_fill_rows_bf16(P(out), P(rg), rows, d, stream()))
    b.done("fill_rows")
    M.assert_bits(M.bits(out), np.broadcast_to(M.bits(row), (rows, d)).copy(), f"fill_rows {rows} x {d}")
    _report("fill_rows_bf16_kernel", (rows, d))


@pytest.mark.parametrize("rows,d", [(11, 300), (1001, 1000)], ids=str)
def test_label_gather_clamps_and_copies(rows, d):
    table = M.random_words((rows, d), rows)
    labels = torch.tensor([0, rows - 1, -1, -(2 ** 31), rows, rows + 5, 2 ** 31 - 1, 3, rows - 2], dtype=torch.int32)
    Bn = len(labels)
    b = Bufs()
    tg, lg, out = b.put(table), b.put(labels), b.out(Bn, d)
    ok(lib().lt_op_label_gather(P(tg), P(lg), P(out), Bn, rows, d, stream()))
    b.done("label_gather")
    M.assert_bits(M.bits(out), M.ref_label_gather(M.bits(table), labels.numpy().astype(np.int64), rows), f"label_gather rows {rows} d {d}")
    _report("label_gather_kernel", (Bn, rows, d))


@pytest.mark.parametrize("n", [0, 1, 1000, 8192 * 256 + 777])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_cast_to_bf16_has_one_correct_word(dtype, n):
    src = M.source(dtype, max(n, 1), 17 * dtype + n % 1000)[:n]
    want, nan = M.convert_words(src)
    b = Bufs()
    sg, out = b.put(src if n else M.source(dtype, 8, 1)), b.out(n + 64)
    ok(lib().lt_op_cast_to_bf16(P(sg), dtype, P(out), n, stream()))
    b.done("cast")
    full, nm = M.sentinel_like((n + 64,)), np.zeros(n + 64, dtype=bool)
    full[:n] = want
    if nan is not None:
        nm[:n] = nan
    M.assert_bits(M.bits(out), full, f"cast_to_bf16 dtype {dtype} n {n}", nm)
    _report("cast_to_bf16_kernel", (dtype, n))


# (rows, cols, dst_ld, r0, row_map)
UPLOAD = [(5, 24, 24, 0, 0), (5, 24, 40, 3, 0), (32, 24, 40, 0, 1), (32, 24, 40, 0, 2), (96, 24, 24, 0, 1), (96, 24, 40, 0, 2), (0, 24, 24, 0, 0), (5, 0, 24, 0, 0),
          (4100, 1024, 1032, 2, 0), (4128, 1024, 1024, 0, 2)]


@pytest.mark.parametrize("c", UPLOAD, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_upload_rows_places_and_converts_every_word(dtype, c):
    rows, cols, ld, r0, rm = c
    n = rows * cols
    src = M.source(dtype, max(n, 1), dtype + sum(c))[:n]
    w, nan = M.convert_words(src)
    dst_rows = (r0 + rows + 2) if rm == 0 else (rows // 32) * 64 + 2
    want, nm = M.ref_upload_rows(w, nan, rows, cols, ld, r0, rm, dst_rows)
    b = Bufs()
    sg, out = b.put(src if n else M.source(dtype, 8, 1)), b.out(dst_rows, ld)
    what = f"upload_rows dtype {dtype} {c}"
    assert rows < 1000 or n > 16384 * 256
    ok(lib().lt_op_upload_rows(P(sg), dtype, P(out), rows, cols, ld, r0, rm, stream()), what)
    b.done(what)
    M.assert_bits(M.bits(out), want, what, nm)
    _report("upload_rows_kernel", (dtype,) + c)


@pytest.mark.parametrize("T,Tpad", [(13, 16), (77, 128), (13, 128)])
def test_mask_to_bias_words(T, Tpad):
    Bn = 4
    g = torch.Generator().manual_seed(T)
    mask = (torch.rand(Bn, T, generator=g) < 0.6).int()
    mask[1] = 0                     # an all-zero row
    mask[2] = 1
    mask[3, 0] = 5                  # any non-zero value is a valid key
    b = Bufs()
    mg, out = b.put(mask), b.out(Bn, Tpad, dtype=torch.float32)
    ok(lib().lt_op_mask_to_bias(P(mg), P(out), Bn, T, Tpad, stream()))
    b.done("mask_to_bias")
    M.assert_bits(M.bits(out), M.ref_mask_to_bias(mask.numpy(), Tpad), f"mask_to_bias T {T} Tpad {Tpad}")
    _report("mask_to_bias_kernel", (Bn, T, Tpad))


# ---- c: rounding chains ---------------------------------------------------------------------------------------------------------------------
def _vals(n, seed, std=1.0):
    return R.draw_rows(1, n, seed, std=std).reshape(-1)


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_add_bf16_is_word_exact(n):
    a, c = _vals(n, n, 1.0), _vals(n, n + 1, 0.3)
    b = Bufs()
    ag, cg, out = b.put(a), b.put(c), b.out(n + 8)
    ok(lib().lt_op_add_bf16(P(ag), P(cg), P(out), n, stream()))
    b.done("add_bf16")
    ch = M.chain_add(a, c)
    share = M.assert_words(out[:n], ch, f"add_bf16 n {n}")
    assert bool((M.bits(out[n:]) == M.SENT16).all())
    _report("add_bf16_kernel", n, share, "sum2 (U)", M.worst_distance(out[:n], ch))


# (out_dtype, B, C, out_ch, H, W, patch, extra ld, use_cfg, cfg_scale, cfg_channels, eol)
UNPATCH = [(1, 2, 4, 4, 16, 16, 2, 0, 0, 1.0, 4, 0), (1, 2, 4, 8, 16, 16, 2, 0, 1, 4.0, 4, 0), (0, 2, 4, 8, 16, 16, 2, 8, 1, 4.0, 3, 0),
           (1, 6, 4, 8, 8, 24, 2, 8, 1, 4.3, 3, 0), (0, 6, 4, 4, 8, 24, 2, 0, 1, 4.3, 4, 1), (1, 2, 4, 8, 8, 24, 2, 8, 0, 1.0, 4, 1),
           (0, 2, 4, 8, 8, 24, 2, 0, 0, 1.0, 4, 0), (1, 2, 4, 8, 8, 24, 2, 0, 1, 4.3, 3, 1), (1, 2, 4, 4, 520, 520, 2, 0, 1, 4.3, 3, 0)]


@pytest.mark.parametrize("c", UNPATCH, ids=lambda c: "-".join(map(str, c)))
def test_unpatchify_cfg_is_word_exact(c):
    od, B, Cc, och, H, W, p, extra, use_cfg, s, cfgc, eol = c
    Hp, Wp = H // p, W // p
    wps = Wp + 1 if eol else 0
    ld = p * p * och + extra
    nrows = B * Hp * (Wp + eol)
    rows = R.draw_rows(nrows, ld, sum(map(int, c[:9])), std=1.0)
    b = Bufs()
    rg, out = b.put(rows), b.out(B * Cc, H * W, dtype=torch.bfloat16 if od else torch.float32)
    what = f"unpatchify_cfg {c}"
    assert H < 100 or B * Cc * H * W > 8192 * 256
    ok(lib().lt_op_unpatchify_cfg(P(rg), ld, P(out), od, B, Cc, och, H, W, p, use_cfg, s, cfgc, wps, stream()), what)
    b.done(what)
    ch = M.ref_unpatchify_cfg(rows, B, Cc, och, H, W, p, use_cfg, s, cfgc, wps)
    share = M.assert_words(out, ch, what) if od else M.assert_f32_holds_bf16(out, ch, what)
    assert torch.equal(rg.cpu(), rows)
    _report("unpatchify_cfg_kernel", c, share, "sum2 (U), fp32 product exact")


# (Y, Hp, Wp, h_split, w_split)
REGION = [(2, 6, 6, 1, 1), (5, 6, 6, 2, 2), (3, 6, 6, 2, 2), (7, 6, 6, 2, 3), (4, 7, 8, 2, 3), (9, 7, 5, 2, 2), (2, 5, 5, 1, 1), (2, 243, 243, 2, 2)]


@pytest.mark.parametrize("c", REGION, ids=lambda c: "-".join(map(str, c)))
def test_region_text_combine_is_word_exact(c):
    Y, Hp, Wp, hs, ws = c
    H, hd = 2, 72
    N, d = Hp * Wp, H * hd
    out0, txt = R.draw_rows(2 * N, d, sum(c), std=1.0), R.draw_rows(Y * N, d, sum(c) + 1, std=1.0)
    for gate in ([20.0, -20.0], [0.0, 0.37], [2.0 ** -9, -1.5]) if N < 1000 else ([0.37, -1.5],):
        gt = torch.tensor(gate).to(torch.bfloat16)
        b = Bufs()
        og, tg, gg = b.put(out0), b.put(txt), b.put(gt)
        what = f"region_text_combine {c} gate {gate}"
        assert N < 1000 or 2 * N * (d // 8) > 8192 * 256
        ok(lib().lt_op_region_text_combine(P(og), P(tg), P(gg), Y, N, H, hd, Hp, Wp, hs, ws, stream()), what)
        b.done(what)
        ch = M.ref_region_text_combine(out0, txt, gt, Y, N, H, hd, Hp, Wp, hs, ws)
        share = M.assert_words(og, ch, what)
        _report("region_text_combine_kernel", c + (tuple(gate),), share, "tanh 40 U, sum2")


@pytest.mark.parametrize("dt", [0.125, -0.0390625, 0.3, -0.0123])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_ode_combine_is_word_exact(mode, dtype, n, dt):
    """bf16 state: the kernel header's chain; fp32 state: numpy float32 operation by operation - ONE word (a contracted multiply-add differs)"""
    g = torch.Generator().manual_seed(mode * 7 + n)
    ts = [torch.randn(n, generator=g) * s for s in (1.0, 0.7, 0.8, 0.9, 0.6)]
    if dtype == 1:
        ts = [t.to(torch.bfloat16) for t in ts]
        dt = float(torch.tensor(dt).to(torch.bfloat16))
    b = Bufs()
    dev = [b.put(t) for t in ts]
    out = b.out(n + 8, dtype=DT[dtype])
    what = f"ode_combine mode {mode} dtype {dtype} n {n} dt {dt}"
    ok(lib().lt_op_ode_combine(mode, *[P(t) for t in dev], P(out), dtype, dt, n, stream()), what)
    b.done(what)
    assert bool((out[n:].cpu().float() == M.SENTINEL).all()), what + ": words past n written"
    if dtype == 1:
        ch = M.ref_ode_combine_bf16(mode, *ts, dt)
        share = M.assert_words(out[:n], ch, what)
        _report("ode_combine_kernel<true>", (mode, n, dt), share, "sum2 (U)")
    else:
        want = M.ref_ode_combine_f32(mode, *ts, dt)
        M.assert_bits(M.bits(out[:n]), want.view(np.int32), what)
        _report("ode_combine_kernel<false>", (mode, n, dt))


@pytest.mark.parametrize("t_index", [0, 2])
@pytest.mark.parametrize("Bn", [1, 2, 8])
@pytest.mark.parametrize("dim", [256, 32, 34])
def test_timestep_features_are_word_exact(dim, Bn, t_index):
    g = torch.Generator().manual_seed(dim + Bn)
    t = torch.rand((t_index + 1) * Bn, generator=g)
    t[t_index * Bn:t_index * Bn + min(3, Bn)] = torch.tensor([0.0, 1.0, 2.0 ** -10])[:min(3, Bn)]
    b = Bufs()
    tg, out = b.put(t), b.out(Bn, dim)
    ok(lib().lt_op_timestep_features(P(tg), t_index, P(out), Bn, dim, stream()))
    b.done("timestep_features")
    ch = M.chain_timestep_features(t[t_index * Bn:(t_index + 1) * Bn], dim)
    share = M.assert_words(out, ch, f"timestep_features dim {dim} B {Bn} t_index {t_index}")
    _report("timestep_features_kernel", (dim, Bn, t_index), share, "TS bound (documented expf / cosf / sinf)", M.worst_distance(out, ch))


# (len, hd, step, theta0, lin0, theta1, lin1, lin_on_pos, out_t)
ROPE = [(384, 72, 4, 10000.0, 2.0, 20000.0, 1.0, 0, 1), (384, 128, 4, 10000.0, 2.0, 20000.0, 1.0, 0, 0), (384, 24, 2, 10000.0, 1.5, 15000.0, 1.0, 1, 1),
        (384, 72, 2, 10000.0, 1.5, 15000.0, 1.0, 1, 0), (1, 72, 4, 10000.0, 2.0, 20000.0, 1.0, 0, 1), (1, 128, 2, 10000.0, 3.0, 500.0, 0.5, 1, 1),
        (384, 128, 2, 10000.0, 1.0, 40000.0, 4.0, 0, 1), (384, 24, 4, 10000.0, 2.0, 20000.0, 1.0, 1, 0)]


@pytest.mark.parametrize("c", ROPE, ids=lambda c: "-".join(map(str, c)))
def test_rope_table_is_within_the_derived_bound(c):
    ln, hd, step, th0, l0, th1, l1, lop, with_t = c
    nf = hd // step
    b = Bufs()
    out = b.out(2, ln, nf, 2, dtype=torch.float32)
    out_t = b.out(2, nf, ln, 2, dtype=torch.float32) if with_t else None
    ok(lib().lt_op_rope_table(P(out), ln, hd, step, th0, l0, th1, l1, lop, stream(), P(out_t)))
    b.done("rope_table")
    val, err = M.ref_rope_table(ln, hd, step, th0, l0, th1, l1, lop)
    worst = M.assert_within(out, val, err, f"rope_table {c}")
    if with_t:
        M.assert_bits(M.bits(out_t), M.bits(out.cpu().permute(0, 2, 1, 3).contiguous()), f"rope_table {c} out_t")
    _report("rope_table_kernel", c, 0.0, "ROPE bound (documented powf / cosf / sinf)", worst)


def _caption(Bn, T, Cc, seed, bf16):
    """caption features in multiples of 2^-6 (|v| < 4: sums over 77 tokens stay far below 2^24 quanta), valid lengths 1, T and one in between"""
    g = torch.Generator().manual_seed(seed)
    cap = torch.randint(-255, 256, (Bn, T, Cc), generator=g).float() / 64.0
    lens = [1, T, max(1, T // 2)][:Bn]
    mask = torch.zeros(Bn, T, dtype=torch.int32)
    for i, n in enumerate(lens):
        mask[i, :n] = 1
    return (cap.to(torch.bfloat16) if bf16 else cap), mask


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("Cc", [64, 300, 2048])
@pytest.mark.parametrize("T", [1, 16, 77])
def test_cap_pool_ln_is_word_exact(T, Cc, bf16):
    Bn = 3
    cap, mask = _caption(Bn, T, Cc, T + Cc, bf16)
    w, bb = R.draw_vec(Cc, Cc + 1, 1.0), R.draw_vec(Cc, Cc + 2, 0.0)
    b = Bufs()
    cg, mg, wg, bg, out = b.put(cap), b.put(mask), b.put(w), b.put(bb), b.out(Bn, Cc)
    what = f"cap_pool_ln T {T} C {Cc} bf16 {bf16}"
    ok(lib().lt_op_cap_pool_ln(P(cg), bf16, P(mg), P(wg), P(bg), P(out), Bn, T, Cc, stream()), what)
    b.done(what)
    share = M.assert_words(out, M.ref_cap_pool_ln(cap, mask, w, bb, bf16), what)
    _report("cap_pool_ln_kernel", (T, Cc, bf16), share, "cap LayerNorm bound")


# (E, d, rows, forced, tie)
ROUTE = [(4, 576, 1, 0, 0), (8, 576, 300, 0, 0), (4, 1536, 300, 0, 0), (8, 1536, 4096, 0, 0), (8, 576, 300, 1, 0), (8, 1536, 300, 0, 1), (4, 576, 300, 0, 1)]


@pytest.mark.parametrize("c", ROUTE, ids=lambda c: "-".join(map(str, c)))
def test_moe_route_is_word_exact(c):
    E, d, rows, forced, tie = c
    x = R.draw_rows(rows, d, sum(c), std=1.0)
    rw = R.draw_vec(E * d, d + E, 0.0, 0.05).view(E, d).clone()
    if tie:                                   # two identical router rows: their logits tie on every token, the lower index must win
        rw[E - 1] = rw[1]
    fz = None
    if forced:
        g = torch.Generator().manual_seed(rows)
        fz = torch.stack([torch.randperm(E, generator=g)[:2] for _ in range(rows)]).int()
    b = Bufs()
    xg, wg, fg = b.put(x), b.put(rw), b.put(fz)
    sel, wts = b.out(rows + 4, 2, dtype=torch.int32), b.out(rows + 4, 2)
    max_tiles = (2 * rows + E * 255 + 255) // 256
    what = f"moe_route {c}"
    ok(lib().lt_op_moe_route(P(xg), P(wg), P(fg), rows, rows, d, E, P(sel), P(wts), max_tiles, stream()), what)
    b.done(what)
    assert bool((sel[rows:].cpu() == int(M.SENTINEL)).all()) and bool((M.bits(wts[rows:]) == M.SENT16).all()), what + ": rows past the end written"
    namb = R.check_routing(x, rw, sel[:rows], wts[:rows], fz, what)
    if tie and not forced:
        s = sel[:rows].cpu()
        assert not bool(((s[:, 0] == E - 1) & (s[:, 1] != 1) | (s[:, 1] == E - 1) & (s[:, 0] != 1)).any()), what + ": the higher index of a tie was chosen without the lower"
    # (as in test_gpu_rows_exact.py the figure printed is the share of ROWS with a logit inside the fp32 dot's bound of a bf16 midpoint: such a row is
    #  compared against every admissible rounding of its logits, each with its own selection and weights - never against a looser rule)
    _report("moe_route_kernel", c, namb / rows, "route_logit_delta, weights 32 U (rows with an ambiguous logit)")


# ---- d: linear_small_m and its extras --------------------------------------------------------------------------------------------------------
ALL_M, ALL_N, ALL_K = [1, 2, 3, 4, 5, 8], [7, 37, 64, 1001], [64, 256, 2048, 560]
PM = (2, 4, 12, 1, 0b0010, 0b0100)         # (L, chunks, d, final, tanh mask, scale mask): 12-column chunks end inside a wave's 8 columns; 96 layer columns,
PM_N = 125                                 # the final layer's chunk 1 at 108..119, five columns past it


def _call_linear(b, a, w, bias, Mr, N, K, act, ext=None, t=None, a2=None, pm=None):
    ag, wg, bg, tg, a2g = b.put(a), b.put(w), b.put(bias), b.put(t), b.put(a2)
    y = b.out(Mr * N + 16)
    if ext:
        L, chunks, pd, fin, tm, sm = pm if pm else (0, 0, 0, -1, 0, 0)
        ok(lib().lt_op_linear_small_m_ext(P(ag), P(wg), P(bg), P(y), Mr, N, K, act, P(tg), P(a2g), L, chunks, pd, fin, tm, sm, stream()), "linear_small_m_ext")
    else:
        ok(lib().lt_op_linear_small_m(P(ag), P(wg), P(bg), P(y), Mr, N, K, act, stream()), "linear_small_m")
    b.done("linear_small_m")
    assert bool((M.bits(y[Mr * N:]) == M.SENT16).all()), "words past M x N written"
    return y[:Mr * N].view(Mr, N)


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("K", ALL_K)
@pytest.mark.parametrize("N", ALL_N)
@pytest.mark.parametrize("Mr", ALL_M)
def test_linear_small_m_silu_and_bias_are_word_exact(Mr, N, K, ext):
    """act_in 1 on silu-safe inputs, weights {-1, 0, 1} 2^e, a bias on every second case: the dot is exact in any order, one rounding follows"""
    seed = Mr * 1000 + N + K
    a = M.draw_silu_inputs(Mr, K, seed)
    w = M.pow2_weights(N, K, seed + 1)
    bias = int_bias(N, torch.Generator().manual_seed(seed)).to(torch.bfloat16) if (Mr + N + K) % 2 else None
    y = _call_linear(Bufs(), a, w, bias, Mr, N, K, 1, ext)
    ch = M.ref_linear_small_m(M.activated(a, None, 1), w, bias)
    M.assert_words(y, ch, f"linear_small_m M {Mr} N {N} K {K} ext {ext} silu")
    _report(f"linear_small_m_kernel<{2 if Mr <= 2 else 4 if Mr <= 4 else 8},{bool(ext)}>", (Mr, N, K, "silu", bias is not None))


@pytest.mark.parametrize("extras", ["a2", "a2+silu", "pm", "a2+silu+pm", "t", "t+a2+pm"])
@pytest.mark.parametrize("Mr", ALL_M)
def test_linear_small_m_extras_are_word_exact(Mr, extras):
    use = set(extras.split("+"))
    K = 256 if "t" in use else 560                     # (256: the engine's feature dimension)
    N = 2 * K + 5 if "t" in use else PM_N
    seed = Mr * 31 + len(extras)
    act = 1 if "silu" in use else 0
    t = a = a2 = None
    if "t" in use:
        t = M.pick_timesteps(K, Mr, seed)
        x = M.chain_timestep_features(t, K).want          # no word ambiguous: the features are known
        w = M.selector_weights(N, K, seed + 1)
        if "a2" in use:                                    # coarse values: feature + a2 must stay unambiguous, checked by activated()
            a2 = (torch.randint(-8, 9, (Mr, K), generator=torch.Generator().manual_seed(seed)).float() / 4).to(torch.bfloat16)
            x = M.activated(x.to(torch.bfloat16), a2, 0)
    else:
        s = M.draw_silu_inputs(Mr, K, seed, grid=2.0 ** -4)
        a, a2 = M.split_sum(s, seed + 2) if "a2" in use else (s, None)
        x = M.activated(a, a2, act)
        w = M.pow2_weights(N, K, seed + 1)
    pm = PM if "pm" in use else None
    y = _call_linear(Bufs(), a, w, None, Mr, N, K, act, 1, t=t, a2=a2, pm=pm)
    ch = M.ref_linear_small_m(x, w, None, pm)
    share = M.assert_words(y, ch, f"linear_small_m_ext M {Mr} {extras}")
    _report(f"linear_small_m_kernel<{2 if Mr <= 2 else 4 if Mr <= 4 else 8},true>", (Mr, N, K, extras), share, "tanh 40 U" if pm else "one word")
