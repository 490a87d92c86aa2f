"""FlowEdit's two chains (transport/edit.py) restated independently of torch's arithmetic: float64 numpy with explicit roundings.

Every operand is a bf16 or fp32 value and every scalar an fp32 value, so the exact result of each single operation is a float64 (a product of two
24-bit significands has 48 bits; a sum or difference is formed in float64 and rounded once more to fp32, which is innocuous for +, -, * at 53 >=
2 * 24 + 2 bits).  ``R`` is the state's rounding: fp32 (ties to even: numpy's float64 -> float32 conversion), then for a bf16 state the nearest
bf16 (ties to even, on the bit pattern)."""
import numpy as np
import torch

from exact_reuse import bf16_round64, f64


def f32_round64(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def rounding(dtype):
    return bf16_round64 if dtype == torch.bfloat16 else f32_round64


def scalars(t, t_next):
    """(t, 1 - t, dt) as the fp32 values the chains multiply by: t an fp32 grid value, the other two formed in double"""
    t, t_next = float(np.float32(t)), float(np.float32(t_next))
    return np.float64(np.float32(t)), np.float64(np.float32(1.0 - t)), np.float64(np.float32(t_next - t))


def mix_chain(x_src, z, noise, t, omt, R):
    """(zs, zt); arrays are float64 images of state-dtype values"""
    zs = R(R(x_src * t) + R(noise * omt))
    return zs, R(zs + R(z - x_src))


def combine_chain(z, out4, w_s, w_t, dt, ch, R, parts=None):
    """z' from the float64 image ``out4 [4 B', C, ...]`` of the evaluation's rows; ``parts`` (a dict) receives v_s, v_t and the exact values in
    front of the three roundings the tie operands aim at"""
    Bp = out4.shape[0] // 4
    c_s, c_t, u_s, u_t = (out4[k * Bp:(k + 1) * Bp] for k in range(4))
    w_s, w_t = np.float64(np.float32(w_s)), np.float64(np.float32(w_t))
    d_s, d_t = R(c_s - u_s), R(c_t - u_t)
    v_s, v_t = R(u_s + R(w_s * d_s)), R(u_t + R(w_t * d_t))
    v_s[:, ch:], v_t[:, ch:] = c_s[:, ch:], c_t[:, ch:]
    step = R(R(v_t - v_s) * dt)
    if parts is not None:
        parts.update(v_s=v_s, v_t=v_t, wd=(w_s * d_s)[:, :ch], dv=v_t - v_s, total=z + step)
    return R(z + step)


def bf16_ties(x):
    """how many exact float64 values lie exactly between two bf16 values"""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    exact = f.astype(np.float64) == x
    return int((exact & ((f.view(np.uint32) & 0xFFFF) == 0x8000)).sum())


def same_words(t, a):
    """a bf16 / fp32 torch tensor equals a float64 array of values of its dtype, word for word (signed zeros included)"""
    got = t.detach().float().cpu().numpy()
    return np.array_equal(got.view(np.uint32), np.asarray(a, dtype=np.float64).astype(np.float32).view(np.uint32))


def tie_operands(dtype=torch.bfloat16):
    """(z, out4, w_s, w_t, dt, ch) with B' = 1, C = 4, ch = 3, 128 pixels, every value a bf16 value, on which a bf16 state meets ties in
    ``w d`` (d = 1 + k / 128 uses all 8 significand bits; 1.5 d and 2.5 d carry 9 or 10), in ``v_t - v_s`` (the unguided channel:
    1 + k / 128 minus an odd multiple of -1 / 256) and in the final sum (z = 1, dt = 1 / 4: steps of m / 512 land between multiples of 1 / 128)"""
    k = torch.arange(128, dtype=torch.float32)
    one = torch.ones(128)
    c_g = 0.5 + k / 128.0
    u_g = -0.5 * one
    c_s = torch.stack([c_g, c_g, c_g.flip(0), -(1.0 + 2.0 * (k % 2)) / 256.0])
    c_t = torch.stack([c_g.flip(0), c_g + 0.25, c_g, 1.0 + k / 128.0])
    u = torch.stack([u_g, u_g, u_g, 0.0 * one])
    out4 = torch.stack([c_s, c_t, u, u]).reshape(4, 4, 1, 128)
    assert torch.equal(out4.to(torch.bfloat16).float(), out4)
    z = torch.ones(1, 4, 1, 128)
    return z.to(dtype), out4.to(dtype), 1.5, 2.5, 0.25, 3


def mix_tie_operands(dtype=torch.bfloat16):
    """(x_src, z, noise, t) of bf16 values: x_src t and noise (1 - t) carry more than 8 significant bits at t = 0.375, half of the products and
    of their sums between two bf16 values; z differs from x_src by one to three bf16 ulps"""
    k = torch.arange(256, dtype=torch.float32)
    x = (1.0 + (k % 128) / 128.0) * torch.where(k < 128, 1.0, -1.0)
    w = (1.0 + ((k * 7) % 128) / 128.0) * torch.where(k % 3 == 0, -1.0, 1.0)
    z = x - (1 + k % 3) / 128.0 * torch.where(x > 0, 1.0, -1.0)  # towards zero: stays on the bf16 grid
    for v in (x, w, z):
        assert torch.equal(v.to(torch.bfloat16).float(), v)
    shape = (1, 4, 8, 8)
    return x.reshape(shape).to(dtype), z.reshape(shape).to(dtype), w.reshape(shape).to(dtype), 0.375
