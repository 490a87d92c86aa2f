"""Guidance reuse restated independently of torch's bf16 arithmetic: float64 numpy with explicit roundings.

Every operand is a bf16 value and the scale an fp32 value, so the exact result of each single operation is a float64: a bf16 has 8 significand
bits and an fp32 24 - a difference or sum of two bf16 values within 2^40 of each other, and the 32-bit product of an fp32 and a bf16, fit the
53 bits of a float64.  The chain's operations are fp32 operations followed by a conversion to bf16; ``R`` below is that pair: the exact value
rounded to fp32 (ties to even: numpy's float64 -> float32 conversion), then to bf16 (ties to even, on the bit pattern)."""
import numpy as np
import torch


def bf16_round64(x):
    """R: an exact float64 result -> fp32 (ties to even) -> nearest bf16 (ties to even), as float64"""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def prod_bf16(w, d):
    """R(w * d): the scale multiplies as an fp32 value"""
    return bf16_round64(np.float64(np.float32(w)) * np.asarray(d, dtype=np.float64))


def refresh_chain(c, u, w):
    """(g, d) of a refresh stage: d = R(c - u), g = R(u + R(w d)); c, u float64 arrays of bf16 values"""
    d = bf16_round64(c - u)
    return bf16_round64(u + prod_bf16(w, d)), d


def reuse_chain(c2, d, w):
    """g of a reuse stage: R(R(c' - d) + R(w d))"""
    return bf16_round64(bf16_round64(c2 - d) + prod_bf16(w, d))


def f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def same_bits(t, a):
    """a bf16 / fp32 torch tensor equals a float64 array of bf16 values, word for word (signed zeros included)"""
    got = t.detach().float().cpu().numpy()
    return np.array_equal(got.view(np.uint32), np.asarray(a, dtype=np.float64).astype(np.float32).view(np.uint32))


def midpoint_operands(w):
    """(c', d) bf16 tensors on which R(w d) and the final sum meet bf16 ties.

    d = 1 + k / 128 (k = 0..127: all 8 significand bits in use): w d for w = 1.5, 2.5, 4.5 carries 9 or 10 significant bits, half of them
    exactly between two bf16 values.  c' is then chosen so that R(c' - d) + R(w d) = 2 R(w d) + e with e one bf16 ulp of the smaller operand:
    sums of 9 significant bits, again ties for every other element."""
    k = torch.arange(128, dtype=torch.float32)
    d = (1.0 + k / 128.0).to(torch.bfloat16)
    assert torch.equal(d.float(), 1.0 + k / 128.0)
    wd = (float(w) * d.float()).to(torch.bfloat16)
    ulp = 2.0 ** -7
    c2 = (d.float() + wd.float() + ulp * (1 + (k % 3))).to(torch.bfloat16)
    return c2, d
