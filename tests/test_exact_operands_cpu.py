"""The exact-operand tier without a GPU: the generators meet the preconditions that make the integer answer the only correct one, the
silu rounding margins hold, and - the point of the tier - `assert_words_equal` fires on every local fault that the global rel-L2
criterion of tests/test_gpu_ops.py lets through."""
import math
import re

import pytest
import torch

import exact_operands as X
import rounding_cases as RC
from grouped_plans import expert_table

# every (K, W density) tests/test_gpu_gemm_exact.py draws: the plain density at all of its K, the SwiGLU W1 densities at theirs
PLAIN_K = [64, 128, 192, 256, 512, 576, 768, 1024, 1152, 1536, 2048, 2304, 3072, 4096, 6144, 8192]
SWIGLU_K = [64, 128, 576, 2304]


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("K", PLAIN_K)
def test_generators_meet_the_preconditions(K, scaled):
    for seed in range(3):
        A, W, _ = X.operands(192, 320, K, _gen(K * 8 + seed), scaled=scaled)
        want = X.expected(A, W)  # raises PreconditionError on any violation; checks 64 rows in int64
        c64 = A.double() @ W.double().t()
        c32 = A.float() @ W.float().t()
        assert torch.equal(c32.double(), c64) and torch.equal(want.double(), c64)
        unscale = 8 if scaled else 1  # the largest output factor is 2^1 * 2^2
        assert float(c64.abs().max()) <= 256 * unscale
        assert float((A.double().abs() @ W.double().abs().t()).max()) * (8 if scaled else 1) < 2 ** 24
        # the draw has the stated densities (to 4 sigma of a binomial)
        for t, d in ((A, X.DENSITY_A), (W, X.DENSITY_W)):
            n = t.numel()
            assert abs(float((t != 0).float().mean()) - d) < 4 * math.sqrt(d * (1 - d) / n)
            assert abs(float(t.float().sign().mean())) < 4 * math.sqrt(d / n)


def test_generators_with_bias_and_the_largest_k():
    A, W, b = X.operands(256, 512, 8192, _gen(1), bias=True)
    assert b is not None and float(b.float().abs().max()) <= 8 and torch.equal(b.float(), b.float().round())
    want = X.expected(A, W, b)
    assert torch.equal(want.double(), A.double() @ W.double().t() + b.double())
    assert float(want.float().abs().max()) <= 256


def test_expected_refuses_operands_that_are_not_exact():
    A, W, _ = X.operands(64, 64, 8192, _gen(2))
    with pytest.raises(X.PreconditionError, match="survive bf16"):
        X.expected(torch.ones(8, 320).bfloat16(), torch.ones(8, 320).bfloat16() + torch.eye(8, 320).bfloat16())  # 321 = 101000001b: 9 bits
    assert X._quantum(torch.tensor([4.0, -6.0, 5.0, 0.0]).double(), "bias") == 1.0  # not the smallest magnitude: the lowest set bit
    assert X._quantum(torch.tensor([0.75, 1.5]).double(), "t") == 0.25 and X._quantum(torch.zeros(3).double(), "t") == 1.0
    with pytest.raises(X.PreconditionError, match="survive bf16"):
        X.expected((A.float() * 0.75).bfloat16(), W)  # 3 * 2^-2 times an integer sum: two more significant bits than bf16 keeps
    with pytest.raises(X.PreconditionError, match="2\\^24"):
        X.expected(torch.tensor([[1.0, 2.0 ** -30]]).bfloat16(), torch.ones(1, 2).bfloat16())  # 1 + 2^-30 does not fit fp32
    big = torch.full((8, 8192), 4096.0)
    big[0, 0] = 2.0 ** -6  # quantum 2^-6, sums near 2^25: 2^31 quanta
    with pytest.raises(X.PreconditionError, match="2\\^24"):
        X.expected(big.bfloat16(), torch.ones(8, 8192).bfloat16())


def test_silu_margin_table():
    """silu(a) for every integer a in [-30, 30] against the bf16 rounding midpoints (float64): the closest is a = -13 at 0.0073 bf16 ulp,
    next a = 2 at 0.016; fp32 and fp64 silu round to the same bf16 word for all of them; the helper's floor of 64 fp32 ulp holds."""
    a = torch.arange(-30, 31, dtype=torch.float64)
    m = X.silu_margins(a)
    order = m.argsort()
    assert int(a[order[0]]) == -13 and abs(float(m[order[0]]) / 65536 - 0.0073) < 1e-4
    assert int(a[order[1]]) == 2 and abs(float(m[order[1]]) / 65536 - 0.016) < 1e-3
    assert float(m.min()) >= X.SILU_MIN_MARGIN_FP32_ULP
    s64 = torch.nn.functional.silu(a).to(torch.bfloat16)
    s32 = torch.nn.functional.silu(a.float()).to(torch.bfloat16)
    assert torch.equal(s64, s32)
    # the margin function itself, on a value that IS a midpoint and on a bf16 value: 1 + 2^-8 lies halfway between 1 and 1 + 2^-7
    x = torch.tensor([1 + 2.0 ** -8, 1.5], dtype=torch.float64)
    m8, e = torch.frexp(x)
    frac = (m8 * 256) - torch.floor(m8 * 256)
    assert float(frac[0]) == 0.5 and float(frac[1]) == 0.0


@pytest.mark.parametrize("K", SWIGLU_K)
def test_swiglu_draws_are_word_exact_with_nothing_masked(K):
    for seed in range(3):
        g = _gen(K + seed)
        A = X.sparse_ints((512, K), X.DENSITY_A, g).bfloat16()
        w1 = X.sparse_ints((256, K), X.w1_density(K), g).bfloat16()
        w3 = X.sparse_ints((256, K), X.DENSITY_W, g).bfloat16()
        want, keep = X.swiglu_expected(A, w1, w3)
        assert bool(keep.all())  # the masked share is 0 for the default draws
        a = A.double() @ w1.double().t()
        b = A.double() @ w3.double().t()
        assert float(a.abs().max()) <= 30
        ref = (torch.nn.functional.silu(a).bfloat16().double() * b).bfloat16()
        assert torch.equal(want, ref)
        assert float((want.float() != 0).float().mean()) > 0.5  # (not a trivial all-zero problem)
    packed = X.pack_w13_ref(w1, w3)
    assert torch.equal(packed[:32], w1[:32]) and torch.equal(packed[32:64], w3[:32]) and torch.equal(packed[64:96], w1[32:64])


# ---- fault sensitivity ------------------------------------------------------------------------------------------------------------
M_, N_, K_ = 1024, 2304, 2304
GEMM_REL_L2_GATE = 4e-3  # tests/test_gpu_ops.py: `assert rel_l2(out, ref) < 4e-3` - quoted, not a new number


def _rel_l2(a, b):  # tests/gpu_util.py
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def exact_problem():
    A, W, _ = X.operands(M_, N_, K_, _gen(M_ + N_ + K_), scaled=True)
    return A, W, X.expected(A, W)


@pytest.fixture(scope="module")
def normal_problem():
    """operands as tests/test_gpu_ops.py draws them and a correct kernel's output: fp32 accumulation, one bf16 rounding"""
    g = _gen(M_ * 7 + N_ * 3 + K_)
    A = torch.randn(M_, K_, generator=g).bfloat16()
    W = (torch.randn(N_, K_, generator=g) / math.sqrt(K_)).bfloat16()
    ref = A.float() @ W.float().t()
    return A, W, ref, ref.bfloat16()


def _box(msg):
    m = re.search(r"rows (\d+)\.\.(\d+), cols (\d+)\.\.(\d+)", msg)
    assert m, msg
    return tuple(int(x) for x in m.groups())


def _fires(got, want):
    with pytest.raises(AssertionError) as e:
        X.assert_words_equal(got, want, "planted")
    return str(e.value)


def test_the_comparator_accepts_the_correct_output(exact_problem):
    _, _, want = exact_problem
    X.assert_words_equal(want.clone(), want, "correct")


@pytest.mark.parametrize("sign,name", [(-1.0, "missing"), (+1.0, "counted twice")])
def test_one_subtile_with_one_slab_missing_or_doubled(exact_problem, normal_problem, sign, name):
    """a 16 x 16 sub-tile whose sum lacks (or repeats) one 32-deep K slab - a ring slot read one slab early or late: caught word-exactly,
    and NOT by the global criterion on random normal operands, which is the gap this tier closes."""
    r0, c0, k0 = 528, 1296, 992
    rows, cols, ks = slice(r0, r0 + 16), slice(c0, c0 + 16), slice(k0, k0 + 32)
    A, W, want = exact_problem
    got = want.clone()
    got[rows, cols] = (want[rows, cols].double() + sign * (A[rows, ks].double() @ W[cols, ks].double().t())).bfloat16()
    msg = _fires(got, want)
    assert _box(msg) == (r0, r0 + 15, c0, c0 + 15), msg
    n_wrong = int(re.search(r"(\d+) of \d+ words wrong", msg).group(1))
    assert 128 < n_wrong <= 256  # (a sparse slab contributes exactly zero to some words)
    assert f"by row % 256 [{r0 % 256}-{r0 % 256 + 15}: {n_wrong}]" in msg and f"by col % 256 [{c0 % 256}-{c0 % 256 + 15}: {n_wrong}]" in msg, msg
    # the suite's criterion so far, on its own kind of operands, with the same fault planted in a correct output
    An, Wn, ref, out = normal_problem
    assert _rel_l2(out, ref) < GEMM_REL_L2_GATE
    bad = out.clone()
    bad[rows, cols] = (ref[rows, cols] + sign * (An[rows, ks].float() @ Wn[cols, ks].float().t())).bfloat16()
    assert not torch.equal(bad, out)
    assert _rel_l2(bad, ref) < GEMM_REL_L2_GATE, f"{name}: the rel-L2 gate does see this fault at this size"  # it does NOT fire


def test_two_adjacent_rows_swapped_inside_a_fragment(exact_problem):
    """a wave's epilogue fragment going to its neighbour's row (over one 256-column tile)"""
    _, _, want = exact_problem
    got = want.clone()
    got[[773, 774], 512:768] = want[[774, 773], 512:768]
    msg = _fires(got, want)
    assert _box(msg) == (773, 774, 512, 767), msg
    assert "by row % 256 [5-6:" in msg, msg


def test_two_32_column_groups_swapped(exact_problem):
    _, _, want = exact_problem
    got = want.clone()
    got[256:512, 1184:1216], got[256:512, 1216:1248] = want[256:512, 1216:1248], want[256:512, 1184:1216]
    msg = _fires(got, want)
    assert _box(msg) == (256, 511, 1184, 1247), msg
    assert "by row % 256 [0-255:" in msg and f"by col % 256 [{1184 % 256}-{1247 % 256}:" in msg, msg


def test_one_word_off_by_one_ulp_and_one_unwritten_word(exact_problem):
    _, _, want = exact_problem
    r, c = 1023, 2303
    assert float(want[r, c]) != 0 or float(want[r, c - 1]) != 0
    if float(want[r, c]) == 0:
        c -= 1
    got = want.clone()
    got.view(torch.int16)[r, c] += 1
    msg = _fires(got, want)
    assert _box(msg) == (r, r, c, c) and "1 of " in msg and "(0 unwritten" in msg, msg
    assert f"({r}, {c}, {float(got[r, c])}, {float(want[r, c])})" in msg, msg
    got = want.clone()
    got[300, 7] = float("nan")
    msg = _fires(got, want)
    assert _box(msg) == (300, 300, 7, 7) and "(1 unwritten" in msg, msg


def test_a_row_tile_computed_with_the_next_experts_weights(exact_problem):
    """grouped launches: a 256-row tile multiplied with the wrong expert's matrix - every expert gets its own integer matrix"""
    A, W, want = exact_problem
    g = _gen(99)
    W_next = X.scale_w(X.sparse_ints((N_, K_), X.DENSITY_W, g)).bfloat16()
    got = want.clone()
    got[512:768] = X.expected(A[512:768], W_next)
    msg = _fires(got, want)
    assert _box(msg) == (512, 767, 0, N_ - 1), msg
    n_wrong = int(re.search(r"(\d+) of \d+ words wrong", msg).group(1))
    assert n_wrong > 0.9 * 256 * N_


def test_keep_mask_and_guarded_buffer():
    want = torch.arange(64, dtype=torch.float32).view(8, 8).bfloat16()
    got = want.clone()
    got[3, 4] += 1
    keep = torch.ones(8, 8, dtype=torch.bool)
    keep[3, 4] = False
    X.assert_words_equal(got, want, "masked", keep=keep)
    with pytest.raises(AssertionError):
        X.assert_words_equal(got, want, "unmasked", keep=torch.ones(8, 8, dtype=torch.bool))
    gb = X.Guarded(5, 8, device="cpu")
    assert gb.out.shape == (5, 8) and bool(torch.isnan(gb.out.float()).all())
    gb.out.copy_(want[:5])
    gb.assert_intact()
    gb.buf[gb.head + 5 * 8 + 3] = 1.0
    with pytest.raises(AssertionError, match="1 behind it \\(first at \\+3 words\\)"):
        gb.assert_intact()


# ---- the final rounding: expected_rounded, its draws, and the faults only it sees -------------------------------------------------------
def test_round_bf16_on_the_bits():
    """ties of both parities, their fp32 neighbours, the largest finite word and the first value that rounds to inf, both signs"""
    bits = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F800000, 0x3F80FFFF, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x00000000]
    bits += [b | 0x80000000 for b in bits]
    x = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)
    want = [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x3F80, 0x3F81, 0x7F7F, 0x7F7F, 0x7F80, 0x7F80, 0x0000]
    want += [w | 0x8000 for w in want]
    got = (X.round_bf16(x).view(torch.int16).to(torch.int64) & 0xFFFF).tolist()
    assert got == want, [hex(g) for g in got]
    assert torch.equal(X.round_bf16(x).view(torch.int16), x.to(torch.bfloat16).view(torch.int16))
    away = (X.round_bf16(x, "away").view(torch.int16).to(torch.int64) & 0xFFFF).tolist()
    assert away[0] == 0x3F81 and away[1] == 0x3F82 and (X.round_bf16(x, "truncate").view(torch.int16).to(torch.int64) & 0xFFFF).tolist()[3] == 0x3F80
    assert float(torch.tensor([0x7F7F], dtype=torch.int16).view(torch.bfloat16).float()) == X.BF16_MAX


def test_expected_rounded_refuses_draws_whose_rounding_does_not_matter():
    A, W, _ = X.operands(64, 64, 256, _gen(3), scaled=True)
    with pytest.raises(X.PreconditionError, match="16 x 16 fragments"):
        X.expected_rounded(A, W)                                        # integer operands: every word exact
    A, W, b = X.rounded_operands(64, 64, 256, _gen(4), 1)
    with pytest.raises(X.PreconditionError, match="share of tie_(even|odd) words"):
        X.expected_rounded(A, W, floors=dict(X.ROUNDING_FLOORS, tie_parity=0.2))
    with pytest.raises(X.PreconditionError, match=r"R\(R\(C\) \+ b\)"):
        X.expected_rounded(A, W, torch.zeros_like(b))                   # a zero bias cannot tell where it is added
    Az = A.clone()
    Az[16:32] = 0
    with pytest.raises(X.PreconditionError, match="16 x 16 fragments"):
        X.expected_rounded(Az, W)
    with pytest.raises(X.PreconditionError, match="2\\^24"):
        X.expected_rounded(A, W, torch.full_like(b.float(), 2.0 ** -40))  # C + bias not exact in fp32
    assert X.amp_a(128) == 57 and X.amp_a(2304) == 12 and X.amp_a(8192) == 6 and 8192 * X.amp_a(8192) * X.AMP_W * 64 < 2 ** 24 * 8


ALL_K = sorted({c[2] for c in RC.PLAIN_CASES} | {c[2] for c in RC.SPLITK_CASES} | {c[4] for c in RC.VT_CASES} | {2304, 6144, 8192})


@pytest.mark.parametrize("K", ALL_K)
@pytest.mark.parametrize("bias_dtype", [None, 0, 1])
def test_rounded_generator_meets_its_floors(K, bias_dtype):
    """three more seeds per K and bias type than the GPU file draws; the stated shares (module comment of exact_operands.py)"""
    for seed in range(3):
        A, W, b = X.rounded_operands(192, 320, K, _gen(K * 8 + seed), bias_dtype)
        info = {}
        want = X.expected_rounded(A, W, b, info=info)
        c32 = A.float() @ W.float().t() + (0 if b is None else b.float())
        assert torch.equal(want, c32.to(torch.bfloat16))                 # fp32 holds the sum exactly: torch's cast of it is the same word
        if b is None:
            assert 0.40 < info["inexact"] < 0.48 and 0.20 < info["tie"] < 0.25 and 0.17 < info["non_tie"] < 0.24, info
        else:
            assert b.dtype == (torch.float32, torch.bfloat16)[bias_dtype] and info["bias_sensitive"] > 0.12, info


# -- every draw of tests/test_gpu_gemm_rounding.py, on the CPU: the GPU machine only runs kernels --
@pytest.mark.parametrize("M,N,K,bias_dtype", sorted({(c[0], c[1], c[2], c[4]) for c in RC.PLAIN_CASES}, key=str))
def test_gpu_draws_plain(M, N, K, bias_dtype):
    RC.plain_problem(M, N, K, bias_dtype, "cpu")


@pytest.mark.parametrize("M,N,K", sorted({c[:3] for c in RC.SWIGLU_CASES} | {c[:3] for c in RC.PAIR_CASES if c[3]}))
def test_gpu_draws_swiglu(M, N, K):
    *_, keep, info = RC.swiglu_problem(M, N // 2, K, "cpu")
    assert info["masked"] <= X.SILU_MAX_MASKED_SHARE and info["skip_a"] >= 0.2 and info["skip_b"] >= 0.12, info


@pytest.mark.parametrize("M,N,K", sorted({(c[0] * c[1], c[2] * c[3], c[4]) for c in RC.VT_CASES} | {(c[0] * c[1], (c[2] + 2 * c[3]) * c[4], c[5]) for c in RC.QKV_CASES} |
                                         {c[:3] for c in RC.PAIR_CASES if not c[3]} | {c[:3] for c in RC.SPLITK_CASES}))
def test_gpu_draws_vt_qkv_pair_splitk(M, N, K):
    RC.plain_problem(M, N, K, None, "cpu")


def test_gpu_draws_grouped_and_top_of_range():
    for epilogue in (0, 1):
        *_, info = RC.grouped_problem(epilogue, "cpu")
        assert info
    c = RC.GROUPED_TAIL
    te = expert_table(4 + c["ntile"] % 5, c["ntile"], [(h * 37 + 1) % c["ntile"] for h in range(c["holes"])], torch.Generator().manual_seed(c["K"] + c["N"] + c["ntile"]))
    g = RC.gen(c["K"], c["N"], c["ntile"])
    A = RC.grouped_a(256 * c["ntile"], c["K"], 0, g)
    W, _ = RC.expert_weights(4 + c["ntile"] % 5, c["N"], c["K"], 0, g)
    RC.grouped_expected(A, W, None, te, 0)
    A, W, want = RC.top_problem("cpu")
    w = want.float()
    assert int(torch.isinf(w).sum()) == 876 and int((w.abs() == X.BF16_MAX).sum()) == 7212 and min(int((w == float("inf")).sum()), int((w == -float("inf")).sum())) >= 256
    assert torch.equal(want, (A.float() @ W.float().t()).to(torch.bfloat16))


def _fp32_sum(t, order):
    """fp32 sum over the last axis in one of three orders: left to right, right to left, pairwise over interleaved lanes"""
    t = t.float()
    if order == "pairwise":
        while t.shape[-1] > 1:
            if t.shape[-1] % 2:
                t = torch.cat([t, torch.zeros_like(t[..., :1])], -1)
            t = t[..., 0::2] + t[..., 1::2]
        return t[..., 0]
    acc = torch.zeros_like(t[..., 0])
    for i in (range(t.shape[-1]) if order == "forward" else reversed(range(t.shape[-1]))):
        acc = acc + t[..., i]
    return acc


def _slot_sums(words32, width, order):
    M, N = words32.shape
    t = torch.nn.functional.pad(words32, (0, (-N) % width)).view(M, -1, width)
    return torch.stack([_fp32_sum(t, order), _fp32_sum(t * t, order)], -1)


STAT_CASES = [("ystat 288-wide tiles", RC.YSTAT["B"] * RC.YSTAT["N"], RC.YSTAT["d"], RC.YSTAT["K"], 144, (1,), None),
              ("ystat 256-wide tiles", RC.YSTAT["B"] * RC.YSTAT["N"], RC.YSTAT["d"], RC.YSTAT["K"], 128, (1,), None),
              ("qstat", RC.QSTAT["B"] * RC.QSTAT["tokens"], 3 * RC.QSTAT["H"] * RC.QSTAT["hd"], RC.QSTAT["K"], 144, (0, 1), RC.QSTAT["H"] * RC.QSTAT["hd"]),
              ("rowstat", RC.ROWSTAT["B"] * RC.ROWSTAT["tokens"], 3 * RC.ROWSTAT["H"] * RC.ROWSTAT["hd"], RC.ROWSTAT["K"], 128, (0, 1), None)]


@pytest.mark.parametrize("name,M,N,K,width,which,q_cols", STAT_CASES)
def test_gpu_draws_statistics_and_their_intervals(name, M, N, K, width, which, q_cols):
    """the discrimination precondition holds on the GPU file's draw; an fp32 sum of the rounded words in three orders lies inside the
    interval (rows sampled: the orders are Python loops); the same sum over the ACCUMULATORS - the planted fault - lies outside, the
    message names the slots, and on integer operands that faulty code gives the exact statistics the existing tests ask for"""
    A, W, want, value, bound, info = RC.stat_problem(M, N, K, width, which, "cpu", q_cols)
    assert all(info[("sum", "sumsq")[i] + "_discriminating"] >= 0.95 for i in which), info
    rows = torch.arange(0, M, max(M // 96, 1))
    q = N if q_cols is None else q_cols
    worst = 0.0
    for order in ("forward", "reverse", "pairwise"):
        got = _slot_sums(want[rows, :q].float(), width, order)
        for i in which:
            stat = {}
            X.assert_stats_within(got[..., i], value[rows][..., i], bound[rows][..., i], f"{name} {order}", stat)
            worst = max(worst, stat["worst_error_over_bound"])
    assert worst <= 1.0
    acc = (A[rows].float() @ W[:q].float().t())                               # exact: what a kernel's accumulators hold
    faulty = _slot_sums(acc, width, "pairwise")
    part = value[rows].clone().float()
    part[:, 1] = faulty[:, 1]                                                # the fault in slot 1 only
    i = which[-1]
    with pytest.raises(AssertionError) as e:
        X.assert_stats_within(part[..., i], value[rows][..., i], bound[rows][..., i], name)
    assert "slots 1..1" in str(e.value) and "by slot [1:" in str(e.value), str(e.value)
    rel = float(((faulty[..., i].double() - value[rows][..., i]).abs() / value[rows][..., i].abs().clamp_min(1e-30)).median())
    assert rel < GEMM_REL_L2_GATE, rel                                        # (and far below any model-level gate)
    Ai, Wi, _ = X.operands(64, width * 2, K, _gen(K + width))
    ci = X.expected(Ai, Wi).double()
    exact = torch.stack([ci.view(64, 2, width).sum(-1), (ci * ci).view(64, 2, width).sum(-1)], -1)
    assert torch.equal(_slot_sums(Ai.float() @ Wi.float().t(), width, "pairwise").double(), exact)   # the integer suite passes the faulty code


# -- a tiled fp32 GEMM on the CPU with the epilogue faults planted --
EM, EN, EK = 192, 384, 512
REGION = (64, 128, 128, 256)   # rows 64..127, cols 128..255: one 64 x 128 tile


def _emulate(A, W, bias=None, order="forward", fault=None):
    """64-deep K slabs accumulated in fp32 (forward / reverse), or four K quarters accumulated apart and summed (split4); bias in fp32;
    one rounding - or `fault`"""
    a, w = A.float(), W.float()
    K = a.shape[1]
    slabs = list(range(0, K, 64))
    groups = {"forward": [slabs], "reverse": [slabs[::-1]], "split4": [slabs[i::4][::-1] for i in range(4)]}[order]
    if fault in ("part_bf16", "sum_bf16"):
        groups = [slabs[i * len(slabs) // 4:(i + 1) * len(slabs) // 4] for i in range(4)]
    parts = []
    for grp in groups:
        acc = torch.zeros(a.shape[0], w.shape[0])
        for k0 in grp:
            acc = acc + a[:, k0:k0 + 64] @ w[:, k0:k0 + 64].t()
        parts.append(acc)
    if fault == "part_bf16":
        parts[2] = X.round_bf16(parts[2]).float()
    if fault == "sum_bf16":
        acc = parts[0]
        for p_ in parts[1:]:
            acc = X.round_bf16(acc + p_).float()
    else:
        acc = parts[0]
        for p_ in parts[1:]:
            acc = acc + p_
    if bias is not None:
        if fault == "bias_late":
            acc = X.round_bf16(acc).float() + bias.float()
        elif fault == "bias_bf16":
            acc = acc + X.round_bf16(bias.float()).float()
        else:
            acc = acc + bias.float()
    return X.round_bf16(acc, {"truncate": "truncate", "away": "away"}.get(fault, "even"))


@pytest.fixture(scope="module")
def rounded_problems():
    out = {}
    for bd in (None, 0, 1):
        A, W, b = X.rounded_operands(EM, EN, EK, _gen(EM + EK + (7 if bd is None else bd)), bd)
        out[bd] = (A, W, b, X.expected_rounded(A, W, b))
    return out


@pytest.mark.parametrize("order", ["forward", "reverse", "split4"])
@pytest.mark.parametrize("bias_dtype", [None, 0, 1])
def test_the_unfaulted_emulation_passes_in_three_summation_orders(rounded_problems, order, bias_dtype):
    A, W, b, want = rounded_problems[bias_dtype]
    X.assert_words_equal(_emulate(A, W, b, order), want, f"emulation {order}")


def _bins_within(msg, axis, lo, hi):
    """every non-empty bin of the message's histogram over `axis` % 256 lies in [lo, hi)"""
    m = re.search(rf"by {axis} % 256 \[([^\]]*)\]", msg)
    assert m, msg
    bins = [int(x) for x in re.findall(r"(\d+)(?=[-:])", m.group(1))]
    assert bins and all(lo <= x < hi for x in bins), msg


GEMM_FAULTS = [("truncate", None), ("away", None), ("bias_late", 0), ("bias_late", 1), ("bias_bf16", 0), ("part_bf16", None), ("sum_bf16", None)]


@pytest.mark.parametrize("fault,bias_dtype", GEMM_FAULTS)
def test_planted_epilogue_fault_is_seen_by_the_rounded_words_only(rounded_problems, fault, bias_dtype):
    """truncation, round-half-away, the bias added after the rounding, an fp32 bias rounded to bf16 before the add, one split-K part
    handed over in bf16, the sum of the parts carried in bf16: (1) the word comparator fires and places the fault when it is planted in
    one 64 x 128 tile; (2) the same code passes the integer-operand check; (3) its rel-L2 to the exact sum stays below the 4e-3 gate"""
    A, W, b, want = rounded_problems[bias_dtype]
    bad = _emulate(A, W, b, "forward", fault)
    share = float((bad != want).double().mean())
    assert share > 0.03, share
    r0, r1, c0, c1 = REGION
    got = want.clone()
    got[r0:r1, c0:c1] = bad[r0:r1, c0:c1]
    msg = _fires(got, want)
    b0, b1, d0, d1 = _box(msg)
    assert r0 <= b0 <= r0 + 8 and r1 - 8 <= b1 < r1 and c0 <= d0 <= c0 + 8 and c1 - 8 <= d1 < c1, msg
    _bins_within(msg, "row", r0, r1)
    _bins_within(msg, "col", c0, c1)
    exact = A.double() @ W.double().t() + (0 if b is None else b.double())
    assert _rel_l2(bad, exact) < GEMM_REL_L2_GATE and _rel_l2(want, exact) < GEMM_REL_L2_GATE, (_rel_l2(bad, exact), _rel_l2(want, exact))
    Ai, Wi, bi = X.operands(EM, EN, EK, _gen(5), scaled=bias_dtype is None, bias=bias_dtype is not None)
    X.assert_words_equal(_emulate(Ai, Wi, bi, "forward", fault), X.expected(Ai, Wi, bi), f"integer operands, fault {fault}")


@pytest.mark.parametrize("skip", ["a", "b"])
def test_swiglu_without_one_of_its_first_two_roundings(skip):
    A, w1, w3 = X.swiglu_rounded_operands(EM, EN // 2, EK, _gen(EK + 1))
    want, keep = X.swiglu_expected_rounded(A, w1, w3)
    a, b = (A.float() @ w1.float().t()).double(), (A.float() @ w3.float().t()).double()    # the emulation's accumulators (exact)
    X.assert_words_equal(X.swiglu_chain(a, b)[0], want, "unfaulted chain", keep=keep)
    bad = X.swiglu_chain(a, b, skip)[0]
    r0, r1, c0, c1 = 64, 128, 64, 128
    got = want.clone()
    got[r0:r1, c0:c1] = bad[r0:r1, c0:c1]
    with pytest.raises(AssertionError) as e:
        X.assert_words_equal(got, want, "planted", keep=keep)
    b0, b1, d0, d1 = _box(str(e.value))
    assert r0 <= b0 and b1 < r1 and c0 <= d0 and d1 < c1 and b1 - b0 > 48 and d1 - d0 > 48, str(e.value)
    assert _rel_l2(bad, want) < GEMM_REL_L2_GATE, _rel_l2(bad, want)             # (the SwiGLU gate of test_gpu_ops.py is 6e-3, against this chain)
    g = _gen(EK + 2)
    Ai, w1i, w3i = X.sparse_ints((EM, EK), X.DENSITY_A, g).bfloat16(), X.sparse_ints((EN // 2, EK), X.w1_density(EK), g).bfloat16(), X.sparse_ints((EN // 2, EK), X.DENSITY_W, g).bfloat16()
    wi, ki = X.swiglu_expected(Ai, w1i, w3i)
    ai, bi = (Ai.float() @ w1i.float().t()).double(), (Ai.float() @ w3i.float().t()).double()
    X.assert_words_equal(X.swiglu_chain(ai, bi, skip)[0], wi, f"integer operands, no R({skip})", keep=ki)
