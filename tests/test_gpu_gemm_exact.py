"""-m gpu: the GEMM family on exact integer operands, EVERY output word compared (helpers and reasoning: exact_operands.py).

On operands in {-1, 0, +1} (times exact powers of two) each product and each partial sum - in any order, with any split of K - is
exact in fp32 and the result is exact in bf16, so the only correct answer is the integer one and the comparison is equality on every
word, at the production shapes, for every kernel.  A fragment that misses one K slab, a row written to its neighbour, a gathered row
from the wrong segment or a K quarter counted twice fails here however large the output is; the rel-L2 tier of test_gpu_ops.py
measures rounding on random operands and cannot see such a fault.  Each dense case first asserts, by lt_op_gemm_describe, WHICH kernel
the launch takes (auto-dispatch names are those of a 256-CU MI355X).  Outputs start as NaN inside a larger allocation whose sentinel
words must survive.  No number from the kernels under test enters an expected value."""
import ctypes as C
import functools

import pytest
import torch

import exact_operands as X
from gpu_util import P, bf, lib, ok, set_option, stream
from grouped_plans import expert_table, filled_row_map, gather_rows, ragged_row_map

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_kernel_variants():
    yield
    set_option("gemm_variant", 0)
    set_option("gemm_splitk", 1)
    set_option("gemm_splitk4", 1)
    set_option("grn_ystat", 1)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _describe(M, N, K, epilogue, variant):
    buf = C.create_string_buffer(200)
    ok(lib().lt_op_gemm_describe(M, N, K, epilogue, variant, buf, 200), "gemm_describe")
    return buf.value.decode()


PLAIN_KERNEL = {1: "gemm_bf16_tn<2,4,4,2,0> ", 2: "gemm_bf16_tn<4,3,2,3,0> ", 3: "gemm_bf16_pp<2,4,4,2,0> ", 7: "gemm_bf16_pp<2,4,2,1,0,",
                8: "gemm_bf16_pp<2,4,1,1,0,", 15: "gemm_bf16_w4q<0,8> ", 16: "gemm_bf16_w4q<0,9> "}
SWIGLU_KERNEL = {1: "gemm_bf16_tn<2,4,4,2,1> ", 3: "gemm_bf16_pp<2,4,4,2,1> ", 7: "gemm_bf16_pp<4,2,1,2,1,", 15: "gemm_bf16_w4q<1,8> "}
VT_KERNEL = {1: "gemm_bf16_tn<2,4,4,2,2> ", 2: "gemm_bf16_tn<4,3,2,3,2> "}
S64, S128, S128_SWIGLU = PLAIN_KERNEL[8], PLAIN_KERNEL[7], SWIGLU_KERNEL[7]
W4Q256, W4Q288, W4Q_SWIGLU = PLAIN_KERNEL[15], PLAIN_KERNEL[16], SWIGLU_KERNEL[15]

TILE_SHAPES = [(256, 256, 64), (300, 576, 128), (257, 296, 192), (130, 32, 576), (1024, 2304, 2304), (512, 512, 6144)]
TILE_AUTO = {(256, 256, 64): S64, (300, 576, 128): S64, (257, 296, 192): S64, (130, 32, 576): S64, (1024, 2304, 2304): S128, (512, 512, 6144): S64}
PERSISTENT_SHAPES = [(8192, 2304, 2304), (8192, 2304, 6144), (8192, 6912, 2304), (8320, 3072, 3072), (8300, 6912, 2304), (70000, 520, 256),
                     (512, 512, 128), (8192, 4096, 4096), (8192, 12288, 4096), (16384, 2304, 6144)]
PERSISTENT_AUTO = {(8192, 2304, 2304): W4Q288, (8192, 2304, 6144): W4Q288, (8192, 6912, 2304): W4Q288, (8320, 3072, 3072): W4Q256,
                   (8300, 6912, 2304): W4Q256, (70000, 520, 256): W4Q288, (512, 512, 128): S64, (8192, 4096, 4096): W4Q256,
                   (8192, 12288, 4096): W4Q256, (16384, 2304, 6144): W4Q288}
SWIGLU_SHAPES = [(256, 128, 64), (300, 1536, 576), (8192, 12288, 2304), (2100, 1280, 128), (256, 131072, 128)]  # M x N = 2 F x K
SWIGLU_AUTO = {(256, 128, 64): S128_SWIGLU, (300, 1536, 576): S128_SWIGLU, (8192, 12288, 2304): W4Q_SWIGLU, (2100, 1280, 128): S128_SWIGLU,
               (256, 131072, 128): W4Q_SWIGLU}


@functools.lru_cache(maxsize=2)
def _dense_problem(M, N, K, with_bias):
    """operands and the expected words of one shape, shared by the variants that run it (one seed per shape)"""
    A, W, b = X.operands(M, N, K, _gen(M * 7 + N * 3 + K + int(with_bias)), scaled=not with_bias, bias=with_bias)
    return A, W, b, X.expected(A, W, b)


@functools.lru_cache(maxsize=1)
def _swiglu_problem(M, F_, K):
    g = _gen(M * 7 + F_ * 3 + K + 2)
    A = X.sparse_ints((M, K), X.DENSITY_A, g).to(torch.bfloat16)
    w1 = X.sparse_ints((F_, K), X.w1_density(K), g).to(torch.bfloat16)
    w3 = X.sparse_ints((F_, K), X.DENSITY_W, g).to(torch.bfloat16)
    want, keep = X.swiglu_expected(A, w1, w3)
    assert bool(keep.all())  # the default draws mask nothing (test_exact_operands_cpu.py)
    return A, w1, w3, want


def _run_dense(A, W, b, want, epilogue, variant, what):
    M, K = A.shape
    N = W.shape[0]
    gb = X.Guarded(M, N // 2 if epilogue else N)
    ok(lib().lt_op_gemm_bf16(P(A), P(W), P(b), 1, P(gb.out), M, N, K, epilogue, variant, stream()), what)
    torch.cuda.synchronize()
    gb.assert_intact(what)
    X.assert_words_equal(gb.out, want, what)


@pytest.mark.parametrize("M,N,K,variant,with_bias", [(*s, v, wb) for s in TILE_SHAPES for wb in (False, True) for v in (0, 1, 2, 3, 7, 8)])
def test_plain_tile_kernels(M, N, K, variant, with_bias):
    """classic 256x256 / 256x288 loops, the 8-wave ping-pong and the two small-M tiles, with and without an integer bias: K = one 64-deep
    block ... 192 ring slabs, ragged both ways, fewer columns than one tile"""
    name = _describe(M, N, K, 0, variant)
    assert name.startswith(PLAIN_KERNEL[variant] if variant else TILE_AUTO[(M, N, K)]), name
    A, W, b, want = _dense_problem(M, N, K, with_bias)
    _run_dense(A, W, b, want, 0, variant, f"{name} {M}x{N}x{K} bias={with_bias}")


@pytest.mark.parametrize("M,N,K,variant", [(*s, v) for s in PERSISTENT_SHAPES for v in (15, 16, 0)])
def test_plain_persistent_kernel(M, N, K, variant):
    """the persistent 4-wave 16x16x32 kernel in its 256- and 288-wide form and what auto-dispatch picks: the 2B and 7B block widths,
    ragged M, many row tiles with ragged N, fewer tiles than CUs with four slabs, several tiles per CU (ring carried across tiles)"""
    name = _describe(M, N, K, 0, variant)
    assert name.startswith(PLAIN_KERNEL[variant] if variant else PERSISTENT_AUTO[(M, N, K)]), name
    A, W, b, want = _dense_problem(M, N, K, False)
    _run_dense(A, W, None, want, 0, variant, f"{name} {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K,variant", [(*s, v) for s in SWIGLU_SHAPES for v in (0, 1, 3, 7, 15)])
def test_swiglu(M, N, K, variant):
    """out = bf16(bf16(silu(w1 x)) * (w3 x)) word for word: with a = w1 x an integer in [-30, 30] both roundings are deterministic, so
    this pins the reference's rounding point between silu and the product, which a 6e-3 rel-L2 cannot.  W packed by lt_op_pack_w13
    (checked against the documented 32-row interleave).  The persistent kernel needs K >= 128: at K = 64 it must refuse the launch."""
    F_ = N // 2
    A, w1, w3, want = _swiglu_problem(M, F_, K)
    packed = torch.full((N, K), float("nan"), device="cuda", dtype=torch.bfloat16)
    ok(lib().lt_op_pack_w13(P(w1), P(w3), P(packed), F_, K, stream()), "pack_w13")
    torch.cuda.synchronize()
    assert torch.equal(packed, X.pack_w13_ref(w1, w3))
    name = _describe(M, N, K, 1, variant)
    if variant == 15 and K < 128:
        assert name == "none", name
        out = torch.empty(M, F_, device="cuda", dtype=torch.bfloat16)
        assert lib().lt_op_gemm_bf16(P(A), P(packed), P(None), 1, P(out), M, N, K, 1, variant, stream()) != 0
        return
    assert name.startswith(SWIGLU_KERNEL[variant] if variant else SWIGLU_AUTO[(M, N, K)]), name
    _run_dense(A, packed, None, want, 1, variant, f"{name} {M}x{N}x{K}")


def _unpair(m):
    """row-major image of a matrix stored row-pair-interleaved (include/lumina_dit.h: (r, k) sits at (r >> 1) * 2 cols + (k >> 5) * 64 +
    (r & 1) * 32 + (k & 31)), by plain indexing"""
    rows, cols = m.shape
    return m.reshape(rows // 2, cols // 32, 2, 32).permute(0, 2, 1, 3).reshape(rows, cols)


@pytest.mark.parametrize("M,N,K,epi,pair_c", [(8192, 2304, 2304, 0, 0), (8192, 2304, 6144, 0, 0), (8192, 6912, 2304, 0, 0), (8192, 12288, 2304, 1, 0),
                                              (8192, 12288, 2304, 1, 1), (8320, 3072, 3072, 0, 0), (8192, 4096, 4096, 0, 0), (8192, 12288, 4096, 0, 0)])
def test_pair_layout(M, N, K, epi, pair_c):
    """the persistent kernel on row-pair-interleaved A and W (converted by lt_op_pair_layout), SwiGLU output row-major and in the pair
    layout: the four block GEMMs of the 2B model at 8192 rows, Flag-DiT's 8320 x 3072 and two d = 4096 shapes"""
    name = _describe(M, N, K, epi, 0)
    assert name.startswith("gemm_bf16_w4q<"), name
    if epi:
        A, w1, w3, want = _swiglu_problem(M, N // 2, K)
        W = X.pack_w13_ref(w1, w3)
    else:
        A, W, _, want = _dense_problem(M, N, K, False)
    Ap, Wp = A.clone(), W.clone()
    ok(lib().lt_op_pair_layout(P(Ap), M, K, 1, stream()))
    ok(lib().lt_op_pair_layout(P(Wp), N, K, 1, stream()))
    torch.cuda.synchronize()
    assert torch.equal(_unpair(Ap), A) and torch.equal(_unpair(Wp), W)
    gb = X.Guarded(M, N // 2 if epi else N)
    ok(lib().lt_op_gemm_bf16_pair(P(Ap), P(Wp), P(gb.out), M, N, K, epi, pair_c, stream()), "gemm pair")
    torch.cuda.synchronize()
    gb.assert_intact(name)
    X.assert_words_equal(_unpair(gb.out) if pair_c else gb.out, want, f"{name} pair {M}x{N}x{K} pair_c={pair_c}")


def _vt_image(cols, B, tokens, kvh, hd):
    """[B * kvh * hd, tokens]: the attention kernels' V image vt[b][h][d][pos(tok)] = cols[b * tokens + tok][h * hd + d] with the key
    permutation inside every 16 keys that swaps bits 2 and 3 of the token index (include/lumina_dit.h, lt_op_v_transpose) - plain indexing"""
    idx = torch.arange(tokens, device=cols.device)
    pos = (idx & ~12) | ((idx & 4) << 1) | ((idx & 8) >> 1)
    v = cols.reshape(B, tokens, kvh, hd).permute(0, 2, 3, 1)
    out = torch.empty_like(v, memory_format=torch.contiguous_format)
    out[..., pos] = v
    return out.reshape(B * kvh * hd, tokens)


@pytest.mark.parametrize("tokens,B,kvh,hd,K,variant", [(4096, 2, 32, 72, 2304, 0), (64, 3, 2, 72, 128, 1), (128, 2, 8, 72, 576, 2),
                                                       (4160, 2, 32, 96, 3072, 0), (1024, 2, 32, 48, 1536, 0), (64, 1, 4, 72, 64, 2),
                                                       (4096, 2, 8, 128, 4096, 0), (4096, 2, 32, 72, 2304, 1), (4096, 2, 32, 72, 2304, 2)])
def test_vt_epilogue(tokens, B, kvh, hd, K, variant):
    M, N = B * tokens, kvh * hd
    name = _describe(M, N, K, 2, variant)
    assert name.startswith(VT_KERNEL[variant]) if variant else name.startswith(tuple(VT_KERNEL.values())), name
    A, W, _, want = _dense_problem(M, N, K, False)
    gb = X.Guarded(B * kvh * hd, tokens)
    ok(lib().lt_op_gemm_vt(P(A), P(W), P(gb.out), M, N, K, tokens, hd, variant, stream()), "gemm_vt")
    torch.cuda.synchronize()
    gb.assert_intact(name)
    X.assert_words_equal(gb.out, _vt_image(want, B, tokens, kvh, hd), f"{name} V^T image [b, h, d] x key")


QKV_SHAPES = [(4096, 2, 32, 32, 72, 2304), (4096, 2, 32, 8, 72, 2304), (1024, 8, 16, 16, 72, 1152), (16384, 1, 32, 8, 72, 256),
              (4160, 2, 32, 32, 96, 3072), (320, 16, 16, 16, 96, 256), (320, 24, 16, 16, 72, 192), (4096, 2, 32, 32, 48, 1536),
              (4096, 2, 32, 8, 128, 4096)]


@pytest.mark.parametrize("tokens,B,H,Hkv,hd,K", QKV_SHAPES)
def test_fused_qkv(tokens, B, H, Hkv, hd, K):
    """one launch of the persistent kernel: plain tiles for the Q | K columns, V^T tiles for the V columns (MHA, GQA, head_dim 48 / 72 /
    96 / 128, samples that end inside a row tile, a ragged last row tile, short K)"""
    M, N, split = B * tokens, H * hd + 2 * Hkv * hd, H * hd + Hkv * hd
    assert lib().lt_op_gemm_qkv_fusable(M, N, K, split, tokens, hd) == 1, "the shape does not take the fused QKV launch"
    A, W, _, want = _dense_problem(M, N, K, False)
    gc, gv = X.Guarded(M, N), X.Guarded(B * Hkv * hd, tokens)
    ok(lib().lt_op_gemm_qkv(P(A), P(W), P(gc.out), P(gv.out), M, N, K, split, tokens, hd, stream()), "gemm_qkv")
    torch.cuda.synchronize()
    gc.assert_intact("C")
    gv.assert_intact("vt")
    X.assert_words_equal(gc.out[:, :split], want[:, :split], "fused QKV, Q | K columns")
    assert bool(torch.isnan(gc.out[:, split:].float()).all()), "the V columns of C were written"
    X.assert_words_equal(gv.out, _vt_image(want[:, split:], B, tokens, Hkv, hd), "fused QKV, V^T image [b, h, d] x key")


@pytest.mark.parametrize("B,tokens,H,Hkv,grid_w", [(2, 4096, 32, 32, 64), (2, 4096, 32, 8, 128)])
def test_qkv_qstat(B, tokens, H, Hkv, grid_w):
    """the fused QKV launch with the row-statistic epilogue (head_dim 72): C and V^T word-exact, and the (mean, rstd) that its K pass reduces
    from the epilogue's partial sums are those of the exact Q columns to fp32 accuracy (the partial sums themselves are exact)"""
    hd = 72
    d, dkv = H * hd, Hkv * hd
    M, N, K, split = B * tokens, d + 2 * dkv, d, d + dkv
    assert lib().lt_op_gemm_qkv_fusable(M, N, K, split, tokens, hd) == 1
    A, W, _, want = _dense_problem(M, N, K, False)
    g = _gen(H * 7 + Hkv)
    kw, kb = bf(1 + 0.1 * torch.randn(dkv, generator=g, device="cuda")), bf(0.1 * torch.randn(dkv, generator=g, device="cuda"))
    table = torch.empty(2, 384, hd // 4, 2, device="cuda", dtype=torch.float32)
    ok(lib().lt_op_rope_table_2d(P(table), 384, hd, 10000.0, 1.0, stream()))
    gc, gv = X.Guarded(M, N), X.Guarded(B * Hkv * hd, tokens)
    k1 = torch.full((B, Hkv, tokens, hd), float("nan"), device="cuda", dtype=torch.bfloat16)
    ws = torch.empty(M, 32, 2, device="cuda", dtype=torch.float32)
    qmr = torch.full((M, 2), float("nan"), device="cuda", dtype=torch.float32)
    ok(lib().lt_op_qkv_qstat(P(A), P(W), P(gc.out), P(gv.out), M, N, K, split, tokens, hd, d, P(kw), P(kb), P(table[1]), grid_w, 0.17,
                             P(k1), P(ws), P(qmr), stream()), "qkv_qstat")
    torch.cuda.synchronize()
    gc.assert_intact("C")
    gv.assert_intact("vt")
    X.assert_words_equal(gc.out[:, :split], want[:, :split], "qkv_qstat, Q | K columns")
    X.assert_words_equal(gv.out, _vt_image(want[:, split:], B, tokens, Hkv, hd), "qkv_qstat, V^T image [b, h, d] x key")
    q = want[:, :d].double()
    mean, var = q.mean(-1), q.var(-1, unbiased=False)
    assert float(((qmr[:, 0].double() - mean).abs() / var.sqrt()).max()) < 1e-5
    assert float((qmr[:, 1].double() * torch.sqrt(var + 1e-5) - 1).abs().max()) < 2e-5
    assert bool(torch.isfinite(k1.float()).all())


SPLITK_CASES = [  # M, N, K, entry point, option gemm_splitk, parts the launch must take (0 = unsplit)
    (512, 1536, 1536, "splitk", 1, 2), (512, 1536, 4096, "splitk", 1, 2), (1024, 2304, 2048, "splitk", 2, 2), (512, 1536, 768, "splitk", 1, 0),
    (500, 1528, 8192, "splitk", 1, 2), (512, 1536, 1536, "auto", 1, 2), (512, 1536, 4096, "auto", 1, 4), (500, 1528, 8192, "auto", 1, 4),
    (512, 1536, 768, "auto", 1, 0), (1024, 2304, 4096, "auto", 1, 0)]


@pytest.mark.parametrize("M,N,K,entry,opt,parts", SPLITK_CASES)
def test_splitk(M, N, K, entry, opt, parts):
    """K split two ways on 64 x 128 tiles (one round, and forced into two rounds), four ways on 128 x 128 tiles, and shapes that must run
    unsplit: the sum of the fp32 parts is exact whatever the arrival order, so every launch gives the integer answer; the workspace says
    which split ran, the counters are back at zero, and a second launch on the same workspace gives the same words"""
    A, W, _, want = _dense_problem(M, N, K, False)
    slots = 256 if entry == "auto" else ((M + 63) // 64) * ((N + 127) // 128)
    part = torch.full((slots * 2 * 64 * 128,), float("nan"), device="cuda", dtype=torch.float32)
    cnt = torch.zeros(slots, device="cuda", dtype=torch.int32)
    fn = lib().lt_op_gemm_splitk_auto if entry == "auto" else lib().lt_op_gemm_splitk
    set_option("gemm_splitk", opt)
    for launch in range(2):
        gb = X.Guarded(M, N)
        ok(fn(P(A), P(W), P(gb.out), M, N, K, P(part), P(cnt), slots, stream()), f"gemm_{entry}")
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0, "a tile counter was left non-zero"
        gb.assert_intact(entry)
        X.assert_words_equal(gb.out, want, f"split-K ({entry}, {parts} parts, launch {launch}) {M}x{N}x{K}")
    t128, t64 = ((M + 127) // 128) * ((N + 127) // 128), ((M + 63) // 64) * ((N + 127) // 128)
    assert int((~torch.isnan(part)).sum()) == {4: t128 * 4 * 128 * 128, 2: t64 * 2 * 64 * 128, 0: 0}[parts]


# ---- grouped (mixture-of-experts) launches ----------------------------------------------------------------------------------------
FILL = 3.0  # rows of padding segments must keep it


def _expert_weights(E, N, K, epilogue, g):
    """one DISTINCT integer matrix per expert: [E, N, K] as the kernel reads it (SwiGLU: packed w1 | w3) and the per-expert parts"""
    if epilogue:
        w1 = X.sparse_ints((E, N // 2, K), X.w1_density(K), g).to(torch.bfloat16)
        w3 = X.sparse_ints((E, N // 2, K), X.DENSITY_W, g).to(torch.bfloat16)
        W = torch.stack([X.pack_w13_ref(w1[e], w3[e]) for e in range(E)])
        return W.contiguous(), (w1, w3)
    W = torch.stack([X.scale_w(X.sparse_ints((N, K), X.DENSITY_W, g)) for _ in range(E)]).to(torch.bfloat16)
    return W.contiguous(), None


def _grouped_expected(A, W, halves, te, epilogue):
    """[M, N or N / 2]: rows of tile t times the matrix of expert te[t]; padding segments keep FILL.  Distinct experts must differ on
    (nearly) every word, or a tile computed with a neighbour's weights could pass."""
    M, No = A.shape[0], W.shape[1] // 2 if epilogue else W.shape[1]
    want = torch.full((M, No), FILL, device=A.device, dtype=torch.bfloat16)
    tile = torch.tensor(te, device=A.device).repeat_interleave(256)
    for e in sorted(set(x for x in te if x >= 0)):
        rows = tile == e
        want[rows] = X.swiglu_expected(A[rows], halves[0][e], halves[1][e])[0] if epilogue else X.expected(A[rows], W[e])
    return want


def _check_grouped(got, want, te, what):
    X.assert_words_equal(got, want, what)
    for t_, ex in enumerate(te):
        if ex < 0:
            assert bool((got[256 * t_: 256 * t_ + 256] == FILL).all()), f"{what}: padding segment {t_} was written"


@pytest.mark.parametrize("variant", [0, 1, 3, 7])
@pytest.mark.parametrize("epilogue", [0, 1])
def test_grouped_expert_segments(variant, epilogue):
    E, K, N = 6, 192, 384
    te = [2, 0, -1, 3, 5, 1, 4, 4]
    M = 256 * len(te)
    g = _gen(17 + epilogue)
    A = (X.sparse_ints((M, K), X.DENSITY_A, g) if epilogue else X.scale_a(X.sparse_ints((M, K), X.DENSITY_A, g))).to(torch.bfloat16)
    W, halves = _expert_weights(E, N, K, epilogue, g)
    want = _grouped_expected(A, W, halves, te, epilogue)
    gb = X.Guarded(M, want.shape[1], fill=FILL)
    tile_expert = torch.tensor(te, dtype=torch.int32, device="cuda")
    ok(lib().lt_op_gemm_grouped(P(A), P(W), P(tile_expert), N * K, P(gb.out), M, N, K, epilogue, variant, stream()), "grouped")
    torch.cuda.synchronize()
    gb.assert_intact("grouped")
    _check_grouped(gb.out, want, te, f"grouped variant {variant} epilogue {epilogue}")


@pytest.mark.parametrize("variant", [0, 3, 7, 15])
@pytest.mark.parametrize("epilogue", [0, 1])
def test_grouped_gather_on_load(variant, epilogue):
    """rows read through the routing plan's inverse map: every token twice, ragged segments, a padding-only tile, -1 rows inside real
    tiles (they read as zero rows)"""
    E, K, N, T = 5, 1536, 512, 600
    te = [2, 2, 0, -1, 3, 1, 4, -1]
    M = 256 * len(te)
    g = _gen(41 + epilogue)
    X_ = X.sparse_ints((T, K), X.DENSITY_A, g).to(torch.bfloat16)
    W, halves = _expert_weights(E, N, K, epilogue, g)
    row_map, cursor = filled_row_map(len(te), {0: 256, 1: 256, 2: 200, 4: 131, 5: 256, 6: 97}, T, torch.Generator().manual_seed(41))
    assert cursor == 2 * T - 4
    want = _grouped_expected(gather_rows(X_, row_map), W, halves, te, epilogue)
    gb = X.Guarded(M, want.shape[1], fill=FILL)
    tile_expert = torch.tensor(te, dtype=torch.int32, device="cuda")
    ok(lib().lt_op_gemm_grouped_gather(P(X_), T, P(row_map.cuda()), P(W), P(tile_expert), N * K, P(gb.out), M, N, K, epilogue, variant, stream()),
       "grouped_gather")
    torch.cuda.synchronize()
    gb.assert_intact("grouped_gather")
    _check_grouped(gb.out, want, te, f"grouped gather variant {variant} epilogue {epilogue}")


@pytest.mark.parametrize("epilogue", [0, 1])
@pytest.mark.parametrize("K,N,ntile,gather", [(512, 4096, 44, True), (1536, 640, 9, True), (256, 2048, 40, False), (4096, 1536, 36, False)])
def test_grouped_persistent_kernel(K, N, ntile, gather, epilogue):
    """grouped mode of the persistent kernel (variant 15): holes anywhere in the table, several tiles per workgroup, ragged N, the
    shortest K the mode accepts, gather-on-load with padding rows inside real tiles; the copy form and the gathered form each against
    the integer answer"""
    E = 4 + ntile % 5
    cpu = torch.Generator().manual_seed(K + N + ntile)
    te = expert_table(E, ntile, (1, ntile // 2, ntile - 1), cpu)
    M = 256 * ntile
    T = M // 2 - 37
    g = _gen(K + N + ntile + epilogue)
    X_ = X.sparse_ints((T, K), X.DENSITY_A, g).to(torch.bfloat16)
    W, halves = _expert_weights(E, N, K, epilogue, g)
    row_map = ragged_row_map(te, T, cpu)
    gathered = gather_rows(X_, row_map)
    want = _grouped_expected(gathered, W, halves, te, epilogue)
    tile_expert = torch.tensor(te, dtype=torch.int32, device="cuda")
    gb = X.Guarded(M, want.shape[1], fill=FILL)
    ok(lib().lt_op_gemm_grouped(P(gathered), P(W), P(tile_expert), N * K, P(gb.out), M, N, K, epilogue, 15, stream()), "grouped w4q")
    torch.cuda.synchronize()
    gb.assert_intact("grouped w4q")
    _check_grouped(gb.out, want, te, f"grouped persistent kernel, copy form, K {K} N {N} {ntile} tiles epilogue {epilogue}")
    if gather:
        gb = X.Guarded(M, want.shape[1], fill=FILL)
        ok(lib().lt_op_gemm_grouped_gather(P(X_), T, P(row_map.cuda()), P(W), P(tile_expert), N * K, P(gb.out), M, N, K, epilogue, 15, stream()),
           "grouped_gather w4q")
        torch.cuda.synchronize()
        gb.assert_intact("grouped_gather w4q")
        _check_grouped(gb.out, want, te, f"grouped persistent kernel, gather-on-load, K {K} N {N} {ntile} tiles epilogue {epilogue}")


@pytest.mark.parametrize("K,N,ntile,holes", [(4096, 1536, 68, 2), (4096, 1536, 64, 0), (1024, 768, 100, 3), (512, 256, 300, 5)])
def test_grouped_tail_split(K, N, ntile, holes):
    """the grouped persistent kernel with the tiles of a partial last round cut along K (2 / 4 parts, picked on the device): tile counts
    that are and are not whole rounds of the CUs; twice on one workspace; counters back at zero"""
    E = 4 + ntile % 5
    te = expert_table(E, ntile, [(h * 37 + 1) % ntile for h in range(holes)], torch.Generator().manual_seed(K + N + ntile))
    M = 256 * ntile
    g = _gen(K + N + ntile)
    A = X.scale_a(X.sparse_ints((M, K), X.DENSITY_A, g)).to(torch.bfloat16)
    W, _ = _expert_weights(E, N, K, 0, g)
    want = _grouped_expected(A, W, None, te, 0)
    tile_expert = torch.tensor(te, dtype=torch.int32, device="cuda")
    cap = 4 * 256
    ws = torch.full((cap, 256 * 256), float("nan"), device="cuda", dtype=torch.float32)
    cnt = torch.zeros(256, device="cuda", dtype=torch.int32)
    valid = sum(1 for x in te if x >= 0) * ((N + 255) // 256)
    tail = valid % 256 if valid > 256 else 0
    for launch in range(2):
        gb = X.Guarded(M, N, fill=FILL)
        ok(lib().lt_op_gemm_grouped_tail(P(A), P(W), P(tile_expert), N * K, P(gb.out), M, N, K, P(ws), P(cnt), cap, stream()), "grouped tail")
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0
        gb.assert_intact("grouped tail")
        _check_grouped(gb.out, want, te, f"grouped tail split K {K} N {N} {ntile} tiles, launch {launch}")
    used = int(torch.isfinite(ws[:, 0]).sum())
    assert used in ((0,) if tail == 0 else (2 * tail, 4 * tail)), (used, tail)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("d,K,N", [(2304, 2304, 4096), (2304, 6144, 4096), (1536, 1536, 8192)])
def test_proj_ystat_epilogue(d, K, N, form):
    """the O / W2 projection on the persistent kernel with the row-statistic epilogue: y word-exact, and the ystat slots of a row add up to
    its sum of y^2 EXACTLY - y is an integer and a row's sum of squares stays below 2^24 (asserted), so every partial is exact in fp32"""
    B = 2
    M = B * N
    A, W, _ = X.operands(M, d, K, _gen(d + K))  # unscaled: y is an integer
    want = X.expected(A, W)
    ysq = want.double().pow(2).sum(-1)
    assert float(ysq.max()) < 2 ** 24
    g = _gen(d + K + 1)
    x = bf(torch.randn(M, d, generator=g, device="cuda"))
    pw, nw = bf(1 + 0.1 * torch.randn(d, generator=g, device="cuda")), bf(1 + 0.1 * torch.randn(d, generator=g, device="cuda"))
    ld = 3 * d
    mod = bf(torch.randn(B, ld, generator=g, device="cuda") * 0.3)
    cap = 2 * ((d + 255) // 256)
    name = _describe(M, d, K, 0, 0)
    assert name.startswith((W4Q256, W4Q288)), name
    gy = X.Guarded(M, d)
    hs = torch.full_like(x, float("nan"))
    ws = torch.full((M, cap), float("nan"), device="cuda", dtype=torch.float32)
    set_option("grn_ystat", form)
    ok(lib().lt_op_proj_gated_residual_norm(P(A), P(W), P(gy.out), P(ws), cap, K, P(x), P(pw), P(mod[:, :d]), P(nw), P(mod[:, d:]), ld, P(hs),
                                            B, N, d, 1e-5, 1, stream()), "proj_gated_residual_norm")
    torch.cuda.synchronize()
    gy.assert_intact(name)
    X.assert_words_equal(gy.out, want, f"{name} with ystat epilogue, y {M}x{d}x{K}")
    nfin = int(torch.isfinite(ws).sum())
    ns = nfin // M
    assert nfin == M * ns and ns == 2 * ((d + (287 if name.startswith(W4Q288) else 255)) // (288 if name.startswith(W4Q288) else 256)), (nfin, M, ns)
    slots = ws.flatten()[: M * ns].view(M, ns).double()
    assert torch.equal(slots, slots.round()) and torch.equal(slots.sum(-1), ysq)
    assert bool(torch.isfinite(x.float()).all()) and bool(torch.isfinite(hs.float()).all())


@pytest.mark.parametrize("M,N,K", [(2, 1000, 256), (2, 9216, 1024), (1, 37, 128), (8, 64, 2048), (3, 1001, 1024), (5, 7, 64), (2, 101376, 1024)])
def test_linear_small_m(M, N, K):
    """the GEMV-style small-M linear (act 0) with an integer bias: N not a multiple of 8 / 32, fewer columns than one wave's eight, every
    register height, the 101 376-column adaLN GEMV"""
    A, W, b = X.operands(M, N, K, _gen(M * 7 + N * 3 + K), bias=True)
    want = X.expected(A, W, b)
    gb = X.Guarded(M, N)
    ok(lib().lt_op_linear_small_m(P(A), P(W), P(b), P(gb.out), M, N, K, 0, stream()), "linear_small_m")
    torch.cuda.synchronize()
    gb.assert_intact("linear_small_m")
    X.assert_words_equal(gb.out, want, f"linear_small_m {M}x{N}x{K}")
