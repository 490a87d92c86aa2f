"""-m gpu: the GEMM epilogues' final fp32 -> bf16 rounding, EVERY output word compared (helpers and reasoning: exact_operands.py,
cases and draws: rounding_cases.py, the draws' floors and the planted faults: test_exact_operands_cpu.py).

test_gpu_gemm_exact.py runs on sums that bf16 holds exactly, so there the last conversion is the identity.  Here the operands carry
integer magnitudes above 1: the exact sum is still ONE fp32 value in any order and with any split of K, but 44 % of the sums need more
than 8 significant bits and 22 % are exact ties, so the one correct word is the round-to-nearest-even of that value and truncation,
round-half-away, a bias added after the rounding (or converted to bf16 before the add), a split-K part handed over in bf16, a statistic
taken from the accumulators or a SwiGLU that skips R(w1 x) / R(w3 x) each change 5 - 27 % of the words.  One case per epilogue code
path at the smallest shapes that reach it; lt_op_gemm_describe asserts which kernel runs.  No number from the kernels under test enters
an expected value."""
import ctypes as C

import pytest
import torch

import exact_operands as X
import rounding_cases as RC
from gpu_util import P, bf, lib, ok, set_option, stream
from grouped_plans import expert_table, filled_row_map, gather_rows
from test_gpu_gemm_exact import PLAIN_KERNEL, SWIGLU_KERNEL, VT_KERNEL, W4Q256, W4Q288, _unpair, _vt_image

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _default_kernel_variants():
    yield
    set_option("gemm_variant", 0)
    set_option("gemm_splitk", 1)
    set_option("gemm_splitk4", 1)
    set_option("grn_ystat", 1)


def _describe(M, N, K, epilogue, variant):
    buf = C.create_string_buffer(200)
    ok(lib().lt_op_gemm_describe(M, N, K, epilogue, variant, buf, 200), "gemm_describe")
    return buf.value.decode()


def _run_dense(A, W, b, want, epilogue, variant, what, keep=None):
    M, K = A.shape
    N = W.shape[0]
    gb = X.Guarded(M, N // 2 if epilogue else N)
    ok(lib().lt_op_gemm_bf16(P(A), P(W), P(b), 0 if b is not None and b.dtype == torch.float32 else 1, P(gb.out), M, N, K, epilogue, variant, stream()), what)
    torch.cuda.synchronize()
    gb.assert_intact(what)
    X.assert_words_equal(gb.out, want, what, keep=keep)


@pytest.mark.parametrize("M,N,K,variant,bias_dtype", RC.PLAIN_CASES)
def test_plain_epilogues(M, N, K, variant, bias_dtype):
    """store_tile of the classic loops, the ping-pong kernel, the two small-M tiles and the persistent kernel: no bias, an fp32 bias with
    12 significant bits, a bf16 bias - added in fp32 BEFORE the one rounding"""
    name = _describe(M, N, K, 0, variant)
    assert name.startswith(PLAIN_KERNEL[variant]), name
    A, W, b, want, _ = RC.plain_problem(M, N, K, bias_dtype, DEV)
    _run_dense(A, W, b, want, 0, variant, f"{name} {M}x{N}x{K} bias dtype {bias_dtype}")


@pytest.mark.parametrize("M,N,K,variant", RC.SWIGLU_CASES)
def test_swiglu_all_four_roundings(M, N, K, variant):
    """out = R(R(silu(R(w1 x))) R(w3 x)) with w1 x on the 2^-8 grid and w3 x an integer, both with more than 8 significant bits"""
    F_ = N // 2
    A, w1, w3, want, keep, _ = RC.swiglu_problem(M, F_, K, DEV)
    packed = torch.full((N, K), float("nan"), device=DEV, dtype=torch.bfloat16)
    ok(lib().lt_op_pack_w13(P(w1), P(w3), P(packed), F_, K, stream()), "pack_w13")
    torch.cuda.synchronize()
    assert torch.equal(packed, X.pack_w13_ref(w1, w3))
    name = _describe(M, N, K, 1, variant)
    assert name.startswith(SWIGLU_KERNEL[variant]), name
    _run_dense(A, packed, None, want, 1, variant, f"{name} {M}x{N}x{K}", keep=keep)


@pytest.mark.parametrize("tokens,B,kvh,hd,K,variant", RC.VT_CASES)
def test_vt_epilogue(tokens, B, kvh, hd, K, variant):
    M, N = B * tokens, kvh * hd
    name = _describe(M, N, K, 2, variant)
    assert name.startswith(VT_KERNEL[variant]), name
    A, W, _, want, _ = RC.plain_problem(M, N, K, None, DEV)
    gb = X.Guarded(B * kvh * hd, tokens)
    ok(lib().lt_op_gemm_vt(P(A), P(W), P(gb.out), M, N, K, tokens, hd, variant, stream()), "gemm_vt")
    torch.cuda.synchronize()
    gb.assert_intact(name)
    X.assert_words_equal(gb.out, _vt_image(want, B, tokens, kvh, hd), f"{name} V^T image [b, h, d] x key")


@pytest.mark.parametrize("tokens,B,H,Hkv,hd,K", RC.QKV_CASES)
def test_fused_qkv(tokens, B, H, Hkv, hd, K):
    """the persistent kernel's fused launch: its plain tiles (Q | K) and its V^T tiles, 256- and 288-wide"""
    M, N, split = B * tokens, H * hd + 2 * Hkv * hd, H * hd + Hkv * hd
    assert lib().lt_op_gemm_qkv_fusable(M, N, K, split, tokens, hd) == 1, "the shape does not take the fused QKV launch"
    A, W, _, want, _ = RC.plain_problem(M, N, K, None, DEV)
    gc, gv = X.Guarded(M, N), X.Guarded(B * Hkv * hd, tokens)
    ok(lib().lt_op_gemm_qkv(P(A), P(W), P(gc.out), P(gv.out), M, N, K, split, tokens, hd, stream()), "gemm_qkv")
    torch.cuda.synchronize()
    gc.assert_intact("C")
    gv.assert_intact("vt")
    X.assert_words_equal(gc.out[:, :split], want[:, :split], "fused QKV, Q | K columns")
    assert bool(torch.isnan(gc.out[:, split:].float()).all()), "the V columns of C were written"
    X.assert_words_equal(gv.out, _vt_image(want[:, split:], B, tokens, Hkv, hd), "fused QKV, V^T image [b, h, d] x key")


@pytest.mark.parametrize("M,N,K,epi,pair_c", RC.PAIR_CASES)
def test_pair_layout(M, N, K, epi, pair_c):
    name = _describe(M, N, K, epi, 0)
    assert name.startswith("gemm_bf16_w4q<"), name
    keep = None
    if epi:
        A, w1, w3, want, keep, _ = RC.swiglu_problem(M, N // 2, K, DEV)
        W = X.pack_w13_ref(w1, w3)
    else:
        A, W, _, want, _ = RC.plain_problem(M, N, K, None, DEV)
    Ap, Wp = A.clone(), W.clone()
    ok(lib().lt_op_pair_layout(P(Ap), M, K, 1, stream()))
    ok(lib().lt_op_pair_layout(P(Wp), N, K, 1, stream()))
    torch.cuda.synchronize()
    assert torch.equal(_unpair(Ap), A) and torch.equal(_unpair(Wp), W)
    gb = X.Guarded(M, N // 2 if epi else N)
    ok(lib().lt_op_gemm_bf16_pair(P(Ap), P(Wp), P(gb.out), M, N, K, epi, pair_c, stream()), "gemm pair")
    torch.cuda.synchronize()
    gb.assert_intact(name)
    X.assert_words_equal(_unpair(gb.out) if pair_c else gb.out, want, f"{name} pair {M}x{N}x{K} pair_c={pair_c}", keep=keep)


@pytest.mark.parametrize("M,N,K,entry,parts", RC.SPLITK_CASES)
def test_splitk_parts_stay_fp32(M, N, K, entry, parts):
    """two-way on 64 x 128 tiles, four-way on 128 x 128 tiles, unsplit: the parts are exact fp32 values and their fp32 sum is the exact
    sum, rounded once - a part stored in bf16 or a running sum carried in bf16 changes 3 - 8 % of the words.  Twice on one workspace."""
    A, W, _, want, _ = RC.plain_problem(M, N, K, None, DEV)
    slots = 256 if entry == "auto" else ((M + 63) // 64) * ((N + 127) // 128)
    part = torch.full((slots * 2 * 64 * 128,), float("nan"), device=DEV, dtype=torch.float32)
    cnt = torch.zeros(slots, device=DEV, dtype=torch.int32)
    fn = lib().lt_op_gemm_splitk_auto if entry == "auto" else lib().lt_op_gemm_splitk
    for launch in range(2):
        gb = X.Guarded(M, N)
        ok(fn(P(A), P(W), P(gb.out), M, N, K, P(part), P(cnt), slots, stream()), f"gemm_{entry}")
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0, "a tile counter was left non-zero"
        gb.assert_intact(entry)
        X.assert_words_equal(gb.out, want, f"split-K ({entry}, {parts} parts, launch {launch}) {M}x{N}x{K}")
    t128, t64 = ((M + 127) // 128) * ((N + 127) // 128), ((M + 63) // 64) * ((N + 127) // 128)
    assert int((~torch.isnan(part)).sum()) == {4: t128 * 4 * 128 * 128, 2: t64 * 2 * 64 * 128, 0: 0}[parts]


def _check_grouped(got, want, keep, te, what):
    X.assert_words_equal(got, want, what, keep=keep)
    for t_, ex in enumerate(te):
        if ex < 0:
            assert bool((got[256 * t_: 256 * t_ + 256] == RC.FILL).all()), f"{what}: padding segment {t_} was written"


@pytest.mark.parametrize("variant", [0, 1, 3, 7, 15])
@pytest.mark.parametrize("epilogue", [0, 1])
def test_grouped_expert_segments(variant, epilogue):
    c = RC.GROUPED
    A, W, want, keep, _ = RC.grouped_problem(epilogue, DEV)
    M = A.shape[0]
    gb = X.Guarded(M, want.shape[1], fill=RC.FILL)
    tile_expert = torch.tensor(c["te"], dtype=torch.int32, device=DEV)
    ok(lib().lt_op_gemm_grouped(P(A), P(W), P(tile_expert), c["N"] * c["K"], P(gb.out), M, c["N"], c["K"], epilogue, variant, stream()), "grouped")
    torch.cuda.synchronize()
    gb.assert_intact("grouped")
    _check_grouped(gb.out, want, keep, c["te"], f"grouped variant {variant} epilogue {epilogue}")


@pytest.mark.parametrize("epilogue", [0, 1])
def test_grouped_gather_on_load_persistent(epilogue):
    c = RC.GROUPED_GATHER
    te, K, N, T = c["te"], c["K"], c["N"], c["T"]
    M = 256 * len(te)
    g = RC.gen(41, epilogue)
    X_ = RC.grouped_a(T, K, epilogue, g).to(DEV)
    W, halves = RC.expert_weights(c["E"], N, K, epilogue, g)
    W = W.to(DEV)
    row_map, _ = filled_row_map(len(te), c["fill"], T, torch.Generator().manual_seed(41))
    # (rows scaled by their position in X_: the gathered rows keep the scale of their source row)
    rows = gather_rows(X_, row_map)
    tile = torch.tensor(te, device=DEV).repeat_interleave(256)
    want = torch.full((M, N // 2 if epilogue else N), RC.FILL, device=DEV, dtype=torch.bfloat16)
    keep = torch.ones_like(want, dtype=torch.bool)
    for e in sorted(set(x for x in te if x >= 0)):
        sel = (tile == e) & (row_map.to(DEV) >= 0)   # padding rows inside a real tile read as zero rows: their words are 0, checked below
        if epilogue:
            want[sel], keep[sel] = X.swiglu_expected_rounded(rows[sel], halves[0][e].to(DEV), halves[1][e].to(DEV))
        else:
            want[sel] = X.expected_rounded(rows[sel], W[e])
        want[(tile == e) & (row_map.to(DEV) < 0)] = 0.0
    gb = X.Guarded(M, want.shape[1], fill=RC.FILL)
    tile_expert = torch.tensor(te, dtype=torch.int32, device=DEV)
    ok(lib().lt_op_gemm_grouped_gather(P(X_), T, P(row_map.to(DEV)), P(W), P(tile_expert), N * K, P(gb.out), M, N, K, epilogue, 15, stream()), "grouped_gather")
    torch.cuda.synchronize()
    gb.assert_intact("grouped_gather")
    _check_grouped(gb.out, want, keep, te, f"grouped gather-on-load, persistent kernel, epilogue {epilogue}")


def test_grouped_tail_split():
    """the tiles of the partial last round cut along K: the parts hand fp32 accumulators over and the last arriver rounds once; twice"""
    c = RC.GROUPED_TAIL
    K, N, ntile = c["K"], c["N"], c["ntile"]
    E = 4 + ntile % 5
    te = expert_table(E, ntile, [(h * 37 + 1) % ntile for h in range(c["holes"])], torch.Generator().manual_seed(K + N + ntile))
    M = 256 * ntile
    g = RC.gen(K, N, ntile)
    A = RC.grouped_a(M, K, 0, g).to(DEV)
    W = RC.expert_weights(E, N, K, 0, g)[0].to(DEV)
    want, _ = RC.grouped_expected(A, W, None, te, 0)
    tile_expert = torch.tensor(te, dtype=torch.int32, device=DEV)
    cap = 4 * 256
    ws = torch.full((cap, 256 * 256), float("nan"), device=DEV, dtype=torch.float32)
    cnt = torch.zeros(256, device=DEV, dtype=torch.int32)
    valid = sum(1 for x in te if x >= 0) * ((N + 255) // 256)
    tail = valid % 256
    assert valid > 256 and tail > 0, "the tile count does not force the split"
    for launch in range(2):
        gb = X.Guarded(M, N, fill=RC.FILL)
        ok(lib().lt_op_gemm_grouped_tail(P(A), P(W), P(tile_expert), N * K, P(gb.out), M, N, K, P(ws), P(cnt), cap, stream()), "grouped tail")
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0
        gb.assert_intact("grouped tail")
        _check_grouped(gb.out, want, None, te, f"grouped tail split, launch {launch}")
    used = int(torch.isfinite(ws[:, 0]).sum())
    assert used in (2 * tail, 4 * tail), (used, tail)


# ---- the statistics epilogues: sums over the bf16-ROUNDED outputs ------------------------------------------------------------------------
STAT_REPORT = {}


@pytest.mark.parametrize("form", [1, 2])
def test_proj_ystat_slots_are_sums_over_the_rounded_words(form):
    """lt_op_proj_gated_residual_norm on the persistent kernel: y word for word, and every half-tile slot of ystat within the fp32
    summation bound of the sum of squares of the expected ROUNDED words (the sum over the accumulators lies outside it for 99 % of the
    slots: asserted on the draw)"""
    c = RC.YSTAT
    B, N, d, K = c["B"], c["N"], c["d"], c["K"]
    M = B * N
    name = _describe(M, d, K, 0, 0)
    assert name.startswith((W4Q256, W4Q288)), name
    width = 144 if name.startswith(W4Q288) else 128
    info = {}
    A, W, want, value, bound, info = RC.stat_problem(M, d, K, width, (1,), DEV)
    g = torch.Generator(device=DEV).manual_seed(d + K + 1)
    x = bf(torch.randn(M, d, generator=g, device=DEV))
    pw, nw = bf(1 + 0.1 * torch.randn(d, generator=g, device=DEV)), bf(1 + 0.1 * torch.randn(d, generator=g, device=DEV))
    ld = 3 * d
    mod = bf(torch.randn(B, ld, generator=g, device=DEV) * 0.3)
    ns = 2 * ((d + 2 * width - 1) // (2 * width))
    cap = ns + 2
    gy = X.Guarded(M, d)
    hs = torch.full_like(x, float("nan"))
    ws = torch.full((M, cap), float("nan"), device=DEV, dtype=torch.float32)
    set_option("grn_ystat", form)
    ok(lib().lt_op_proj_gated_residual_norm(P(A), P(W), P(gy.out), P(ws), cap, K, P(x), P(pw), P(mod[:, :d]), P(nw), P(mod[:, d:]), ld, P(hs),
                                            B, N, d, 1e-5, 1, stream()), "proj_gated_residual_norm")
    torch.cuda.synchronize()
    gy.assert_intact(name)
    X.assert_words_equal(gy.out, want, f"{name} with ystat epilogue, y {M}x{d}x{K}")
    assert int(torch.isfinite(ws).sum()) == M * ns, (int(torch.isfinite(ws).sum()), M, ns)
    slots = ws.flatten()[: M * ns].view(M, ns)
    X.assert_stats_within(slots, value[..., 1], bound[..., 1], f"ystat form {form}, slots of {width} columns", info)
    print(f"ystat form {form}: {name}; discriminating slots {info['sumsq_discriminating']:.4f}; worst error / bound {info['worst_error_over_bound']:.4f}")
    assert bool(torch.isfinite(x.float()).all()) and bool(torch.isfinite(hs.float()).all())


def test_qkv_qstat_slots_and_mean_rstd():
    """lt_op_qkv_qstat: C and V^T word for word; the (sum, sum of squares) partials of its workspace within the fp32 bound of the sums over
    the expected ROUNDED Q words; (mean, rstd) those of the rounded Q columns (bounds of test_gpu_gemm_exact.test_qkv_qstat)"""
    c = RC.QSTAT
    B, tokens, H, Hkv, hd, K, grid_w = (c[k] for k in ("B", "tokens", "H", "Hkv", "hd", "K", "grid_w"))
    d, dkv = H * hd, Hkv * hd
    M, N, split = B * tokens, d + 2 * dkv, d + dkv
    assert lib().lt_op_gemm_qkv_fusable(M, N, K, split, tokens, hd) == 1
    g = torch.Generator(device=DEV).manual_seed(H * 7 + Hkv)
    kw, kb = bf(1 + 0.1 * torch.randn(dkv, generator=g, device=DEV)), bf(0.1 * torch.randn(dkv, generator=g, device=DEV))
    table = torch.empty(2, 384, hd // 4, 2, device=DEV, dtype=torch.float32)
    ok(lib().lt_op_rope_table_2d(P(table), 384, hd, 10000.0, 1.0, stream()))
    gc, gv = X.Guarded(M, N), X.Guarded(B * Hkv * hd, tokens)
    k1 = torch.full((B, Hkv, tokens, hd), float("nan"), device=DEV, dtype=torch.bfloat16)
    ws = torch.full((M * 32, 2), float("nan"), device=DEV, dtype=torch.float32)
    qmr = torch.full((M, 2), float("nan"), device=DEV, dtype=torch.float32)
    A, W, _, want, _ = RC.plain_problem(M, N, K, None, DEV)
    ok(lib().lt_op_qkv_qstat(P(A), P(W), P(gc.out), P(gv.out), M, N, K, split, tokens, hd, d, P(kw), P(kb), P(table[1]), grid_w, 0.17,
                             P(k1), P(ws), P(qmr), stream()), "qkv_qstat")
    torch.cuda.synchronize()
    gc.assert_intact("C")
    gv.assert_intact("vt")
    X.assert_words_equal(gc.out[:, :split], want[:, :split], "qkv_qstat, Q | K columns")
    X.assert_words_equal(gv.out, _vt_image(want[:, split:], B, tokens, Hkv, hd), "qkv_qstat, V^T image [b, h, d] x key")
    written = int((~torch.isnan(ws[:, 0])).sum())
    assert written % M == 0 and bool((~torch.isnan(ws[:written])).all()), "the written slots are not one dense [M][slots] block"
    slots = written // M
    assert slots > 0 and (2 * d) % slots == 0 and 2 * d // slots in (256, 288), (slots, d)
    width = d // slots
    *_, value, bound, info = RC.stat_problem(M, N, K, width, (0, 1), DEV, q_cols=d)
    X.assert_stats_within(ws[:written].view(M, slots, 2), value, bound, f"qstat partials, slots of {width} columns", info)
    print(f"qstat: slots of {width}; discriminating {info['sum_discriminating']:.4f} / {info['sumsq_discriminating']:.4f}; worst error / bound {info['worst_error_over_bound']:.4f}")
    q = want[:, :d].double()
    mean, var = q.mean(-1), q.var(-1, unbiased=False)
    assert float(((qmr[:, 0].double() - mean).abs() / var.sqrt()).max()) < 1e-5
    assert float((qmr[:, 1].double() * torch.sqrt(var + 1e-5) - 1).abs().max()) < 2e-5
    assert bool(torch.isfinite(k1.float()).all())


def test_rowstat_slots_are_sums_over_the_rounded_words():
    """the small-M QKV projection in front of the fused small attention (lt_op_qkv_attention_small hands its workspace back): C word for
    word, every 128-column (sum, sum of squares) within the fp32 bound of the sums over the expected ROUNDED words"""
    from exact_prologue import quarter_turn_table
    c = RC.ROWSTAT
    B, tokens, H, Hkv, hd, K, grid_w = (c[k] for k in ("B", "tokens", "H", "Hkv", "hd", "K", "grid_w"))
    d, dkv = H * hd, Hkv * hd
    M, N = B * tokens, d + 2 * dkv
    A, W, want, value, bound, info = RC.stat_problem(M, N, K, 128, (0, 1), DEV)
    ones, zeros = bf(torch.ones(d)), bf(torch.zeros(d))
    table, _ = quarter_turn_table(2, 40, hd, 1, DEV)
    slots = (N + 127) // 128
    Cg = X.Guarded(M, N)
    ws = torch.full((M, slots, 2), float("nan"), device=DEV, dtype=torch.float32)
    out = X.Guarded(M, d)
    ok(lib().lt_op_qkv_attention_small(P(A), P(W), P(Cg.out), M, K, H, Hkv, tokens, hd, P(ones), P(zeros), P(ones), P(zeros), P(table), 40, grid_w, 1.0,
                                       P(ws), P(out.out), stream()), "qkv_attention_small")
    torch.cuda.synchronize()
    Cg.assert_intact("C")
    out.assert_intact("out")
    X.assert_words_equal(Cg.out, want, "small-M QKV GEMM with the rowstat epilogue")
    X.assert_stats_within(ws, value, bound, "rowstat, 128-column tiles", info)
    print(f"rowstat: discriminating {info['sum_discriminating']:.4f} / {info['sumsq_discriminating']:.4f}; worst error / bound {info['worst_error_over_bound']:.4f}")


# ---- the top of the range ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", RC.TOP_VARIANTS)
def test_top_of_the_range(variant):
    """sums between the largest finite bf16 and 2^128 (finite in fp32; every product of one sign per row, so no partial sum overflows):
    below the halfway point the largest finite word, at or above it +-inf - and never a NaN"""
    M, N, K = RC.TOP_SHAPE
    name = _describe(M, N, K, 0, variant)
    assert name.startswith(PLAIN_KERNEL[variant]), name
    A, W, want = RC.top_problem(DEV)
    _run_dense(A, W, None, want, 0, variant, f"{name} top of the range")
