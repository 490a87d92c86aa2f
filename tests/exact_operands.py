"""Exact-operand GEMM checks: generators, the expected value and the word-exact comparator (plain module, no test in here).

bf16 GEMM with fp32 accumulation on operands in {-1, 0, +1} (times exact powers of two) has ONE correct answer: every product and
every partial sum, in any order and with any split of K, is an integer multiple of a common power of two that fits fp32's 24 bits,
and the result fits bf16's 8.  So a kernel is compared with `torch.equal` on every output word - independent of summation order,
tile walk, split-K arrival order and MFMA shape - and a single wrong 16 x 16 fragment anywhere in an 8192 x 12288 output is a failure.

`expected()` checks the preconditions on every call (a draw that violates one is an ERROR of the test, never a looser comparison):
  * every operand is an integer multiple of its power-of-two quantum and max sum_k |a w| / (quantum_A quantum_W) < 2^24
    (=> every partial sum, in any order, is exact in fp32);
  * every expected word survives a round trip through bf16;
  * 64 rows of it, recomputed on the CPU in int64, agree with the float64 matmul (the reference does not rest on a vendor GEMM alone).

That answer makes the epilogue's fp32 -> bf16 conversion the identity.  `expected_rounded()` is the second expected value: the same exact
fp32 sum on operands with integer magnitudes above 1 (`rounded_operands`), where a large share of the sums needs more than 8
significant bits, and the ONE correct word is the round-to-nearest-even bf16 of that one fp32 value (ties to even, no neighbour passes),
computed on the integer bits and cross-checked against torch's CPU cast.  Every draw asserts that the rounding matters (`ROUNDING_FLOORS`).
"""
import math

import torch

DENSITY_A = 1 / 2
DENSITY_W = 1 / 4
FP32_EXACT = float(1 << 24)
SILU_MIN_MARGIN_FP32_ULP = 64.0   # 2^-18 relative: the fused epilogue's fp32 silu (exp2 + rcp) is good to ~2.5e-6 relative at |a| = 30
SILU_MAX_MASKED_SHARE = 0.01
SENTINEL = 7.0


class PreconditionError(RuntimeError):
    """the drawn operands do not make the integer answer the only correct one"""


# ---- generators -----------------------------------------------------------------------------------------------------------------
def sparse_ints(shape, density, gen, amp=1):
    """float32 tensor on the generator's device, entries +1 / -1 with probability density / 2 each, else 0; amp > 1: the non-zero entries
    times an integer magnitude uniform in [1, amp] (amp <= 255: exact in bf16)"""
    r = torch.rand(shape, generator=gen, device=gen.device)
    s = (r < density / 2).to(torch.float32) - (r >= 1 - density / 2).to(torch.float32)
    if amp > 1:
        assert amp <= 255
        s = s * torch.randint(1, amp + 1, shape, generator=gen, device=gen.device).to(torch.float32)
    return s


def scale_rows(m, period, bias_exp):
    """row r times 2^(r % period - bias_exp): exact, and a row swapped with its neighbour changes magnitude as well as value"""
    e = (torch.arange(m.shape[0], device=m.device) % period - bias_exp).to(torch.float32)
    return m * torch.exp2(e).unsqueeze(1)


def scale_a(A):
    return scale_rows(A, 3, 1)


def scale_w(W):
    return scale_rows(W, 5, 2)


def int_bias(N, gen):
    return torch.randint(-8, 9, (N,), generator=gen, device=gen.device).to(torch.float32)


def operands(M, N, K, gen, scaled=False, bias=False, density_a=DENSITY_A, density_w=DENSITY_W):
    """(A [M, K], W [N, K], bias [N] or None) in bf16 on the generator's device.  Cases with a bias use the unscaled operands: an
    integer added to a scaled sum can need more than 8 significant bits."""
    assert not (scaled and bias)
    A = sparse_ints((M, K), density_a, gen)
    W = sparse_ints((N, K), density_w, gen)
    if scaled:
        A, W = scale_a(A), scale_w(W)
    b = int_bias(N, gen).to(torch.bfloat16) if bias else None
    return A.to(torch.bfloat16).contiguous(), W.to(torch.bfloat16).contiguous(), b


def w1_density(K):
    """W1 half of a SwiGLU problem: a = w1 x has variance K * DENSITY_A * density, held at <= 16 (|a| <= 30 is 7.5 sigma)"""
    return min(1 / 16, 32 / K)


# ---- expected value -------------------------------------------------------------------------------------------------------------
def _quantum(t, what):
    """the largest power of two every entry of t is an integer multiple of (1 for an all-zero tensor)"""
    nz = t[t != 0].abs()
    if nz.numel() == 0:
        return 1.0
    q = 2.0 ** math.floor(math.log2(float(nz.min())))
    for _ in range(24):  # bf16 values carry 8 significant bits: a few halvings reach the lowest set bit
        s = nz / q
        if bool((s == s.round()).all()):
            return q
        q /= 2
    raise PreconditionError(f"{what}: entries share no power-of-two quantum within 24 bits of the smallest magnitude")


def _exact_sum(A, W, bias=None, sample_rows=64):
    """float64 [M, N] = A W^T (+ bias) on A's device after the quantum / 2^24 precondition and the int64 cross-check of sampled rows: the
    value is exact in fp32, and so is every partial sum in any order and with any split of K"""
    Ad, Wd = A.double(), W.double()
    unit = _quantum(Ad, "A") * _quantum(Wd, "W")
    C = Ad @ Wd.t()
    S = Ad.abs() @ Wd.abs().t()
    if bias is not None:
        bd = bias.double()
        unit = min(unit, _quantum(bd, "bias"), 1.0) if bool((bd != 0).any()) else unit
        C += bd
        S += bd.abs()
    worst = float(S.max()) / unit
    if not worst < FP32_EXACT:
        raise PreconditionError(f"max sum_k |a w| = {worst} quanta >= 2^24: a partial sum could round in fp32")
    del S
    # 64 rows again, in int64 on the CPU
    M = A.shape[0]
    idx = torch.unique(torch.linspace(0, M - 1, min(sample_rows, M)).round().long())
    qa, qw = _quantum(Ad, "A"), _quantum(Wd, "W")
    ai = (Ad[idx.to(A.device)] / qa).round().long().cpu()
    wi = (Wd / qw).round().long().cpu()
    ci = (wi @ ai.t().contiguous()).t()   # [rows, N], quanta of qa * qw
    have = C[idx.to(A.device)].cpu()
    if bias is not None:
        have = have - bias.double().cpu()
    if not torch.equal((have / (qa * qw)).round().long(), ci) or not torch.equal(ci.double() * (qa * qw), have):
        raise PreconditionError("float64 matmul and int64 matmul disagree on the sampled rows")
    return C


def expected(A, W, bias=None, sample_rows=64):
    """bf16 [M, N] = A W^T (+ bias) by float64 matmul on A's device, after the precondition checks of the module docstring."""
    C = _exact_sum(A, W, bias, sample_rows)
    want = C.to(torch.bfloat16)
    if not torch.equal(want.double(), C):
        bad = int((want.double() != C).sum())
        raise PreconditionError(f"{bad} expected words do not survive bf16 (max |C| = {float(C.abs().max())})")
    return want


def silu_margins(a_values):
    """for integer a: distance of silu(a) (float64) from the nearest bf16 rounding midpoint, in fp32 ulp of silu(a).  bf16 keeps 8
    significant bits, fp32 24: one bf16 ulp = 2^16 fp32 ulp, a midpoint sits at an odd multiple of 2^15 fp32 ulp."""
    a = torch.as_tensor(a_values, dtype=torch.float64)
    s = a / (1 + torch.exp(-a))
    out = torch.full_like(s, float("inf"))
    nz = s != 0
    m, e = torch.frexp(s[nz].abs())          # |s| = m 2^e, m in [0.5, 1)
    in_bf16_ulp = m * 256                     # [128, 256): bf16 ulp = 1 here
    frac = in_bf16_ulp - torch.floor(in_bf16_ulp)
    out[nz] = (frac - 0.5).abs() * 65536.0    # fp32 ulp
    return out


def swiglu_expected(A, w1, w3):
    """(want bf16 [M, F], keep bool [M, F]) for out = bf16(bf16(silu(w1 x)) * (w3 x)), the reference's rounding points.  a = w1 x and
    b = w3 x are exact integers; the product of two bf16 values is exact in fp32, so its rounding is deterministic, and silu's is
    wherever silu(a) is not within the kernel's fp32 evaluation error of a bf16 midpoint: `keep` is False for an `a` whose margin is
    below SILU_MIN_MARGIN_FP32_ULP (none in [-30, 30]: tests/test_exact_operands_cpu.py) and |a| <= 30 is required outright."""
    a = expected(A, w1).double()
    b = expected(A, w3).double()
    if float(a.abs().max()) > 30:
        raise PreconditionError(f"|w1 x| reaches {float(a.abs().max())} > 30: draw W1 sparser")
    vals = torch.unique(a)
    margin = silu_margins(vals.cpu())
    weak = vals[(margin < SILU_MIN_MARGIN_FP32_ULP).to(vals.device)]
    keep = ~torch.isin(a, weak)
    if float((~keep).double().mean()) > SILU_MAX_MASKED_SHARE:
        raise PreconditionError(f"{float((~keep).double().mean()):.3%} of the SwiGLU outputs sit on a silu rounding midpoint")
    s32, s64 = torch.nn.functional.silu(a.float()).to(torch.bfloat16), torch.nn.functional.silu(a).to(torch.bfloat16)
    if not torch.equal(s32[keep], s64[keep]):
        raise PreconditionError("fp32 and fp64 silu round to different bf16 words")
    want = (s64.float() * b.float()).to(torch.bfloat16)   # bf16 x bf16 is exact in fp32: one deterministic rounding
    return want, keep


def pack_w13_ref(w1, w3):
    """the packed [2F, K] layout of the SwiGLU epilogue (include/lumina_dit.h): 32-row groups alternate w1 / w3"""
    F_, K = w1.shape
    return torch.stack([w1.view(F_ // 32, 32, K), w3.view(F_ // 32, 32, K)], 1).reshape(2 * F_, K).contiguous()



# ---- the final rounding: operands whose sums bf16 cannot hold -----------------------------------------------------------------------
# Integer magnitudes: W in [-AMP_W, AMP_W], A in [-amp_a(K), amp_a(K)], densities as above.  The sum of K products has the standard
# deviation sigma = sqrt(K DENSITY_A DENSITY_W E[a^2] E[w^2]) quanta, E[x^2] = (amp + 1)(2 amp + 1) / 6 for a uniform magnitude; amp_a(K)
# is the largest amplitude with sigma <= SIGMA_QUANTA.  Among the integers of [2^(8 + j), 2^(9 + j)) a share 2^-(j + 1) is exact in bf16,
# 2^-(j + 1) are ties and the rest is neither, so sigma = 600 (about a third of the sums below 256, a quarter in [256, 512), a third in
# [512, 1024)) gives all three classes a two-digit share at every K; max sum_k |a w| <= K amp_a(K) AMP_W < 2^20 quanta for K <= 8192.
AMP_W = 7
SIGMA_QUANTA = 600.0
# floors every draw must meet (shares of the output words; measured shares per case: profiles/gemm_rounding/TABLE.md - the smallest over the
# suite's draws are 0.42 inexact, 0.22 ties (0.16 with a bf16 bias), 0.11 per tie parity, 0.20 non-tie, 0.16 bias-sensitive; with the
# 12-bit fp32 bias 0.86 inexact, 0.088 ties, 0.76 non-tie)
ROUNDING_FLOORS = dict(inexact=0.35, tie=0.12, tie_parity=0.04, non_tie=0.15)
ROUNDING_FLOORS_FP32_BIAS = dict(inexact=0.80, tie=0.04, tie_parity=0.015, non_tie=0.70)   # 12-bit bias: most words inexact, fewer ties
BIAS_SENSITIVE_FLOOR = 0.05   # share of words with R(R(C) + b) != R(C + b)
STAT_DISCRIMINATING_FLOOR = 0.85
BF16_MAX = float.fromhex("0x1.fep127")


def _mean_square(amp):
    return (amp + 1) * (2 * amp + 1) / 6


def amp_a(K):
    amp = 1
    while amp < 127 and K * DENSITY_A * DENSITY_W * _mean_square(amp + 1) * _mean_square(AMP_W) <= SIGMA_QUANTA ** 2:
        amp += 1
    return amp


def rounded_operands(M, N, K, gen, bias_dtype=None):
    """(A [M, K], W [N, K] bf16, bias [N] or None) with the row scalings of scale_a / scale_w.  The bias is an integer multiple of the
    output quantum 2^-3 (rows of A start at 2^-1, rows of W at 2^-2) whose magnitudes span those of the sums of its column (the scalings
    spread them over 2^0 ... 2^6 quanta times sigma).  bias_dtype 1: bf16, 2^(n % 7 - 3) m with |m| <= 255; 0: fp32 with 12 significant
    bits, 2^(n % 3 - 3) m with |m| <= 4095 - a bias that a conversion to bf16 before the add would change."""
    A = scale_a(sparse_ints((M, K), DENSITY_A, gen, amp_a(K)))
    W = scale_w(sparse_ints((N, K), DENSITY_W, gen, AMP_W))
    b = None
    if bias_dtype is not None:
        m = torch.randint(-255, 256, (N,), generator=gen, device=gen.device) if bias_dtype else torch.randint(-4095, 4096, (N,), generator=gen, device=gen.device)
        e = (torch.arange(N, device=gen.device) % (7 if bias_dtype else 3) - 3).to(torch.float32)
        b = (m.to(torch.float32) * torch.exp2(e)).to(torch.bfloat16 if bias_dtype else torch.float32)
    return A.to(torch.bfloat16).contiguous(), W.to(torch.bfloat16).contiguous(), b


def top_of_range_operands(M, N, K, device):
    """sums n 2^117 with n = 2000 + r % 24 + (7 c) % 24 (sign by row parity): the largest finite bf16 is 2040 2^117, the halfway point to
    2^128 = 2048 2^117 is 2044 2^117.  Every product is positive (negative in odd rows), so no partial sum, in any order, leaves the range of the
    final one: 125 terms of 16 spread over K, one of r % 24 and one of (7 c) % 24."""
    assert K >= 128
    A, W = torch.zeros(M, K, device=device), torch.zeros(N, K, device=device)
    ks = torch.unique(torch.linspace(0, K - 3, 125).round().long())[:125]
    ks = torch.arange(K - 2)[:125] if ks.numel() < 125 else ks
    A[:, ks], W[:, ks] = 1.0, 16.0
    free = [k for k in range(K) if k not in set(ks.tolist())]
    A[:, free[0]], W[:, free[0]] = (torch.arange(M, device=device) % 24).float(), 1.0
    A[:, free[-1]], W[:, free[-1]] = 1.0, (torch.arange(N, device=device) * 7 % 24).float()
    A = A * (1 - 2 * (torch.arange(M, device=device) % 2)).float().unsqueeze(1)
    return (A * 2.0 ** 58).to(torch.bfloat16), (W * 2.0 ** 59).to(torch.bfloat16)


def round_bf16(x32, mode="even"):
    """bf16 of a finite fp32 tensor by integer arithmetic on the bits.  'even': round to nearest, ties to even (the one correct word);
    'truncate' and 'away' (ties away from zero) are the planted faults of tests/test_exact_operands_cpu.py"""
    assert x32.dtype == torch.float32 and bool(torch.isfinite(x32).all())
    u = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = {"even": (u + 0x7FFF + ((u >> 16) & 1)) >> 16, "away": (u + 0x8000) >> 16, "truncate": u >> 16}[mode] & 0xFFFF
    return (r - ((r & 0x8000) << 1)).to(torch.int16).view(torch.bfloat16)


def _as_fp32(C, what):
    c32 = C.float()
    if not torch.equal(c32.double(), C) or not bool(torch.isfinite(c32).all()):
        raise PreconditionError(f"{what}: the exact value is not a finite fp32 number")
    return c32


def rounding_shares(c32):
    """shares of the words of an fp32 tensor whose bf16 rounding is not the identity, is an exact tie (kept bit even / odd), is neither"""
    u = c32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    low, odd = u & 0xFFFF, ((u >> 16) & 1).bool()
    tie = low == 0x8000
    n = float(u.numel())
    return dict(inexact=float((low != 0).sum()) / n, tie=float(tie.sum()) / n, tie_even=float((tie & ~odd).sum()) / n,
                tie_odd=float((tie & odd).sum()) / n, non_tie=float(((low != 0) & ~tie).sum()) / n), low != 0


def _require_rounding_matters(c32, floors, what):
    sh, inexact = rounding_shares(c32)
    frag = torch.nn.functional.max_pool2d(inexact.float()[None, None], 16, ceil_mode=True)
    if not bool((frag > 0).all()):
        raise PreconditionError(f"{what}: {int((frag == 0).sum())} 16 x 16 fragments of the output hold no inexact word")
    for key, floor in (("inexact", floors["inexact"]), ("tie", floors["tie"]), ("tie_even", floors["tie_parity"]), ("tie_odd", floors["tie_parity"]),
                       ("non_tie", floors["non_tie"])):
        if not sh[key] >= floor:
            raise PreconditionError(f"{what}: share of {key} words {sh[key]:.4f} below the floor {floor}")
    return sh


def expected_rounded(A, W, bias=None, sample_rows=64, floors="draw", info=None):
    """bf16 [M, N]: round-to-nearest-even of the exact fp32 value A W^T (+ bias; C + bias exact in fp32 too), preconditions as expected().
    floors (None for the hand-built draws that assert their own conditions): the draw must make the rounding matter.  With a bias,
    R(R(C) + b) must differ from R(C + b) on BIAS_SENSITIVE_FLOOR of the words.  info: a dict that receives the measured shares."""
    if floors == "draw":
        floors = ROUNDING_FLOORS_FP32_BIAS if bias is not None and bias.dtype == torch.float32 else ROUNDING_FLOORS
    C = _exact_sum(A, W, bias, sample_rows)
    c32 = _as_fp32(C, "A W^T + bias")
    want = round_bf16(c32)
    cpu = c32.cpu().to(torch.bfloat16)
    if not torch.equal(want.cpu().view(torch.int16), cpu.view(torch.int16)):
        raise PreconditionError("integer round-to-nearest-even and torch's CPU cast disagree")
    sh = _require_rounding_matters(c32, floors, "A W^T + bias") if floors is not None else rounding_shares(c32)[0]
    if bias is not None:
        c0 = _as_fp32(C - bias.double(), "A W^T")
        late = round_bf16(round_bf16(c0).float() + bias.float())   # (a bf16 + fp32 sum that is not exact rounds once more: still a fault)
        sh["bias_sensitive"] = float((late != want).sum()) / want.numel()
        if floors is not None and not sh["bias_sensitive"] >= BIAS_SENSITIVE_FLOOR:
            raise PreconditionError(f"R(R(C) + b) differs from R(C + b) on {sh['bias_sensitive']:.4f} of the words only")
    if info is not None:
        info.update(sh)
    return want


# SwiGLU: A as above without the row scaling, w1 = integers in [-8, 8] at density 1 / 2 times 2^-8, so a = w1 x lies on the 2^-8 grid
# (up to 13 significant bits at |a| = 30) with the variance K / 4 (amp_a^2 / 3)(25.5) 2^-16 <= 16 by amp_a's sigma rule; w3 as W above.
SWIGLU_W1_AMP, SWIGLU_W1_DENSITY, SWIGLU_W1_EXP = 8, 1 / 2, -8
SWIGLU_SKIP_FLOOR = dict(a=0.20, b=0.12)   # share of output words that change when R(a) / R(b) is skipped (measured 0.26 - 0.27 / 0.17: TABLE.md)


def swiglu_rounded_operands(M, F_, K, gen):
    A = sparse_ints((M, K), DENSITY_A, gen, amp_a(K))
    w1 = sparse_ints((F_, K), SWIGLU_W1_DENSITY, gen, SWIGLU_W1_AMP) * 2.0 ** SWIGLU_W1_EXP
    w3 = sparse_ints((F_, K), DENSITY_W, gen, AMP_W)
    return A.to(torch.bfloat16).contiguous(), w1.to(torch.bfloat16).contiguous(), w3.to(torch.bfloat16).contiguous()


def swiglu_chain(a, b, skip=None):
    """the reference's four rounding points on exact fp32 a = w1 x, b = w3 x (float64 tensors): a' = R(a), b' = R(b), s = R(silu(a')),
    out = R(s b') -> (out bf16, a' float64).  skip 'a' / 'b': that rounding left out, as a kernel that feeds its fp32 accumulator on"""
    a1 = a if skip == "a" else round_bf16(a.float()).double()
    b1 = b if skip == "b" else round_bf16(b.float()).double()
    s = torch.nn.functional.silu(a1).to(torch.bfloat16)
    return round_bf16((s.double() * b1).float()), a1   # bf16 x bf16 is exact in fp32; s x fp32 takes the one fp32 rounding a kernel's would


def swiglu_expected_rounded(A, w1, w3, info=None):
    """(want bf16 [M, F], keep bool [M, F]): swiglu_expected's rules on sums that need more than 8 bits - |a| <= 30, the silu margin over
    the distinct a', at most SILU_MAX_MASKED_SHARE masked - and the draw must make the first two roundings matter"""
    a = _exact_sum(A, w1)
    b = _exact_sum(A, w3)
    _as_fp32(a, "w1 x"), _as_fp32(b, "w3 x")
    if float(a.abs().max()) > 30:
        raise PreconditionError(f"|w1 x| reaches {float(a.abs().max())} > 30: draw W1 sparser")
    want, a1 = swiglu_chain(a, b)
    vals = torch.unique(a1)
    margin = silu_margins(vals.cpu())
    weak = vals[(margin < SILU_MIN_MARGIN_FP32_ULP).to(vals.device)]
    keep = ~torch.isin(a1, weak)
    masked = float((~keep).double().mean())
    if masked > SILU_MAX_MASKED_SHARE:
        raise PreconditionError(f"{masked:.3%} of the SwiGLU outputs sit on a silu rounding midpoint")
    s32, s64 = torch.nn.functional.silu(a1.float()).to(torch.bfloat16), torch.nn.functional.silu(a1).to(torch.bfloat16)
    if not torch.equal(s32[keep], s64[keep]):
        raise PreconditionError("fp32 and fp64 silu round to different bf16 words")
    sh = dict(masked=masked, a_inexact=rounding_shares(a.float())[0]["inexact"], b_inexact=rounding_shares(b.float())[0]["inexact"])
    for skip in ("a", "b"):
        other = swiglu_chain(a, b, skip)[0]
        sh["skip_" + skip] = float(((other != want) & keep).sum()) / want.numel()
        if not sh["skip_" + skip] >= SWIGLU_SKIP_FLOOR[skip]:
            raise PreconditionError(f"skipping R({skip}) changes {sh['skip_' + skip]:.4f} of the words only")
    if info is not None:
        info.update(sh)
    return want, keep


# ---- the statistics epilogues -------------------------------------------------------------------------------------------------------
def slot_stats(words, width):
    """words float64 [M, N] -> (value, bound) [M, slots, 2]: per `width`-column slot the float64 (sum, sum of squares) and the worst case
    of an fp32 summation of those terms in ANY order, n_terms 2^-24 sum |term| (n - 1 additions, each rounding a partial sum that is at
    most sum |term| to half an ulp; a bf16 word and its square are exact fp32 terms)"""
    M, N = words.shape
    t = torch.nn.functional.pad(words, (0, (-N) % width)).view(M, -1, width)
    n = torch.nn.functional.pad(torch.ones(N, dtype=torch.float64, device=words.device), (0, (-N) % width)).view(-1, width).sum(-1)
    value = torch.stack([t.sum(-1), (t * t).sum(-1)], -1)
    bound = torch.stack([t.abs().sum(-1), (t * t).sum(-1)], -1) * (n * 2.0 ** -24).view(1, -1, 1)
    return value, bound


def expected_slot_stats(want, unrounded, width, what, which=(0, 1), info=None):
    """slot_stats of the expected ROUNDED words, after the precondition that the same statistic over the unrounded sums lies outside the
    accepted interval for STAT_DISCRIMINATING_FLOOR of the (row, slot) pairs - a kernel that reduced its accumulators would fail"""
    value, bound = slot_stats(want.double(), width)
    other, _ = slot_stats(unrounded, width)
    for i in which:
        share = float(((other[..., i] - value[..., i]).abs() > bound[..., i]).double().mean())
        if info is not None:
            info[("sum", "sumsq")[i] + "_discriminating"] = share
        if not share >= STAT_DISCRIMINATING_FLOOR:
            raise PreconditionError(f"{what}: the {('sum', 'sum of squares')[i]} over the unrounded sums lies outside the interval for {share:.3f} of the slots only")
    return value, bound


def assert_stats_within(got, value, bound, what, info=None):
    """got [M, slots] or [M, slots, k] (fp32) inside value +- bound; the message names the slots: count, bounding box, worst error as a
    fraction of the bound, histogram by row % 256 and by slot"""
    g = got.double()
    err = (g - value).abs()
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    frac = torch.where(torch.isnan(g), torch.full_like(frac, float("inf")), frac)
    if info is not None:
        info["worst_error_over_bound"] = float(frac.max())
    bad = frac > 1
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero()
    hr = torch.bincount(idx[:, 0] % 256, minlength=256).cpu()
    hs = torch.bincount(idx[:, 1], minlength=256).cpu()
    first = [(tuple(i), float(g[tuple(i)]), float(value[tuple(i)]), float(bound[tuple(i)])) for i in idx[:4].tolist()]
    raise AssertionError(f"{what}: {n} of {bad.numel()} statistics outside their interval (worst {float(frac.max()):.3g} x the bound); rows "
                         f"{int(idx[:, 0].min())}..{int(idx[:, 0].max())}, slots {int(idx[:, 1].min())}..{int(idx[:, 1].max())}; first (index, got, want, "
                         f"bound) {first}; by row % 256 {_runs(hr)}; by slot {_runs(hs)}")


# ---- comparator -----------------------------------------------------------------------------------------------------------------
def _runs(hist):
    """'16-31: 256' style summary of the non-empty bins of a 256-bin histogram"""
    out, i, n = [], 0, hist.numel()
    h = hist.tolist()
    while i < n:
        if h[i] == 0:
            i += 1
            continue
        j = i
        while j + 1 < n and h[j + 1] != 0:
            j += 1
        out.append(f"{i}-{j}: {sum(h[i:j + 1])}" if j > i else f"{i}: {h[i]}")
        i = j + 1
    return "[" + ", ".join(out[:12]) + (", ..." if len(out) > 12 else "") + "]"


def wrong_words(got, want, keep=None):
    """bool [M, N]: words of got that differ from want in value (NaN - an unwritten word - differs from everything)"""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.bfloat16, (got.shape, want.shape, got.dtype, want.dtype)
    bad = ~(got == want)
    if keep is not None:
        bad &= keep
    return bad


def assert_words_equal(got, want, what="", keep=None):
    """torch.equal on the bf16 words of two [M, N] tensors; the failure message names the fragment: count, bounding box, the first few
    (row, col, got, want), and the wrong-word histogram folded by row % 256 and col % 256."""
    if keep is None and torch.equal(got, want):
        return
    bad = wrong_words(got, want, keep)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero()
    r0, r1, c0, c1 = int(idx[:, 0].min()), int(idx[:, 0].max()), int(idx[:, 1].min()), int(idx[:, 1].max())
    first = [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in idx[:6].tolist()]
    hr = torch.bincount(idx[:, 0] % 256, minlength=256).cpu()
    hc = torch.bincount(idx[:, 1] % 256, minlength=256).cpu()
    nan = int(torch.isnan(got.float())[bad].sum())
    raise AssertionError(f"{what}: {n} of {bad.numel()} words wrong ({nan} unwritten / NaN); rows {r0}..{r1}, cols {c0}..{c1}; "
                         f"first (row, col, got, want) {first}; by row % 256 {_runs(hr)}; by col % 256 {_runs(hc)}")


class Guarded:
    """an [M, N] bf16 output pre-filled with NaN inside an ordinary larger allocation whose head (256 words) and tail (256 more rows'
    worth of words + 64) hold a sentinel that must survive the launch - stray stores past M or N land there."""

    def __init__(self, M, N, device="cuda", fill=float("nan")):
        self.head, self.n = 256, M * N
        tail = 256 * N + 64
        self.buf = torch.full((self.head + self.n + tail,), SENTINEL, device=device, dtype=torch.bfloat16)
        self.out = self.buf[self.head:self.head + self.n].view(M, N)
        self.out.fill_(fill)

    def assert_intact(self, what=""):
        lo, hi = self.buf[:self.head], self.buf[self.head + self.n:]
        nlo, nhi = int((lo != SENTINEL).sum()), int((hi != SENTINEL).sum())
        if nlo or nhi:
            first = int((hi != SENTINEL).nonzero()[0]) if nhi else -1
            raise AssertionError(f"{what}: stray stores outside the output: {nlo} words before it, {nhi} behind it (first at +{first} words)")
