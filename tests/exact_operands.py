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
def sparse_ints(shape, density, gen):
    """float32 tensor on the generator's device, entries +1 / -1 with probability density / 2 each, else 0"""
    r = torch.rand(shape, generator=gen, device=gen.device)
    return (r < density / 2).to(torch.float32) - (r >= 1 - density / 2).to(torch.float32)


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


def expected(A, W, bias=None, sample_rows=64):
    """bf16 [M, N] = A W^T (+ bias) by float64 matmul on A's device, after the precondition checks of the module docstring."""
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
    want = C.to(torch.bfloat16)
    if not torch.equal(want.double(), C):
        bad = int((want.double() != C).sum())
        raise PreconditionError(f"{bad} expected words do not survive bf16 (max |C| = {float(C.abs().max())})")
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
