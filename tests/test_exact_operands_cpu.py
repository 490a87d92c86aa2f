"""The exact-operand tier without a GPU: the generators meet the preconditions that make the integer answer the only correct one, the
silu rounding margins hold, and - the point of the tier - `assert_words_equal` fires on every local fault that the global rel-L2
criterion of tests/test_gpu_ops.py lets through."""
import math
import re

import pytest
import torch

import exact_operands as X

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
