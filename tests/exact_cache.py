"""Restatements the step-caching tests compare with: the bf16 chains of the residual kernels, operands that sit on their rounding
edges, the float64 indicator sums and the bounds a summation order is worth."""
import torch

U = 2.0 ** -53  # unit roundoff of float64


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def bf_from_bits(words):
    return torch.tensor(words, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


def ref_store(xl, x0):
    """r = bf16(xl - x0): fp32 from the bf16 words, one rounding"""
    return (xl.float() - x0.float()).to(torch.bfloat16)


def ref_apply_x(x0, r):
    """x = bf16(x0 + r)"""
    return (x0.float() + r.float()).to(torch.bfloat16)


def edge_operands(n, seed):
    """two bf16 vectors of n words: random draws, then overwritten from the front with pairs whose sum / difference cancels, lands on a bf16
    midpoint (ties to even, both parities), is +-0, or leaves the bf16 range"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=g).mul(3).to(torch.bfloat16)
    b = torch.randn(n, generator=g).mul(3).to(torch.bfloat16)
    top = 3.3895313892515355e38  # the largest finite bf16
    pairs = [(1.0, 1.0), (1.0, -1.0), (-2.5, 2.5),               # cancelling: +0 either way
             (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 0.0),  # signed zeros
             (1.0, 2.0 ** -8), (1.0, -(2.0 ** -9)),               # 1 + 2^-8: midpoint of 1 and 1 + 2^-7 -> even (1); 1 - 2^-9: midpoint below 1
             (1.0078125, 2.0 ** -8), (1.0078125, -(2.0 ** -8)),   # odd mantissa: the tie goes up / down to the even neighbour
             (256.0, 1.0), (256.0, -0.5), (257.0 - 1.0, 3.0),     # midpoints at another exponent, and past one
             (top, top), (top, -top), (-top, -top), (top, 2.0 ** 119), (top, 2.0 ** 120),  # the top of the range: overflow, cancel, the last tie
             (2.0 ** -126, -(2.0 ** -126)), (2.0 ** -133, 2.0 ** -133)]  # the bottom: smallest normal, a subnormal
    assert n >= len(pairs)
    for i, (p, q) in enumerate(pairs):
        a[i], b[i] = p, q
    return a, b


def integer_operands(n, seed, lim=64):
    """bf16 integers in [-lim, lim]: every |a - b| and every partial sum is an integer float64 holds exactly"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-lim, lim + 1, (n,), generator=g).to(torch.bfloat16)
    b = torch.randint(-lim, lim + 1, (n,), generator=g).to(torch.bfloat16)
    return a, b


def ref_sums(h, h_prev):
    """(S1, S0) in float64 by torch's reduction"""
    a, b = h.double().reshape(-1).cpu(), h_prev.double().reshape(-1).cpu()
    return float((a - b).abs().sum()), float(b.abs().sum())


def chain_depth(n):
    """the longest chain of additions one term goes through in cache_indicator_kernel's order for n words: the 8-word chunks a thread walks
    (ceil(n / 8 / (512 * 256)) of them, 8 terms each), 6 lane steps, 3 wave adds, 7 block adds in the finishing wave and its 6 lane steps"""
    chunks = -(-n // 8)
    per_thread = -(-chunks // (512 * 256))
    return 8 * per_thread + 6 + 3 + 7 + 6


def sum_bound(n):
    """RELATIVE distance allowed between the kernel's float64 sum of n non-negative terms and torch's: n 2^-53, as the issue states it.
    Derivation: a summation whose longest addition chain has depth k is within k u (1 + O(k u)) of the exact sum, relative, when no term is
    negative (Higham, Accuracy and Stability, 4.2: a term meets at most k roundings, and sum |x_i| IS the sum).  The kernel's k is
    chain_depth(n) = 8 ceil(n / 2^20) + 22, which leaves torch's sum n - chain_depth(n) roundings of the budget: 34 at n = 64, the smallest
    shape the tests use, where torch's vectorised reduction adds 64 terms through a chain of at most 4 lanes' partial sums + 16 serial steps."""
    assert n >= 64 and chain_depth(n) + 20 <= n
    return n * U


def rel_bound(n):
    """... and rel = S1 / S0 formed from two such pairs of sums: each quotient carries both sums' distances and its own rounding"""
    return 2.0 * sum_bound(n) + 2.0 * U
