"""What the masked (inpainting) sampler computes (helper of tests/test_masked_cpu.py and tests/test_gpu_masked.py; plain module, no test in here).

``known`` and ``blend`` are the torch expressions of the host loop that defines the feature (transport/masked.py), on whatever device the
tensors live on: PyTorch's own type promotion and kernels decide every rounding.  ``t`` is a Python float - ``float(tgrid[i + 1])`` in the loop.

``chain64`` restates the same arithmetic without torch's promotion rules: numpy float64, one operation at a time, each result rounded to fp32
(the op-math format of every elementwise kernel) and then to the state dtype D.  A float64 product of an fp32 and a D operand is exact, a float64
sum of two is exact or rounds once at 53 bits, which the following rounding to 24 bits hides (53 >= 2 * 24 + 2): every stage is the ONE correct
word, there is no ambiguity to carry.

    R(R(step m) + R(R(R(noise (1 - t)) + R(x1 t)) R(1 - m)))        1 - t: double, then fp32;  t: fp32;  1 - m: a tensor op in D
"""
import numpy as np
import torch


def known(noise, x1, t):
    return noise * (1 - t) + x1 * t  # the expression of sample_img2img.py (z = z * (1 - t0) + x1 * t0), t a Python float


def blend(step, m, noise, x1, t):
    return step * m + known(noise, x1, t) * (1 - m)


def _bf16_round64(x):
    """float64 array holding fp32 values -> the nearest bf16 value (ties to even), by integer arithmetic on the fp32 word"""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).astype(np.float64)


def chain64(step, m, noise, x1, t, dtype):
    """the blend in float64 with the rounding points stated one by one; operands are tensors of the state dtype; returns a tensor of it"""
    f64 = lambda v: v.detach().cpu().to(torch.float64).numpy()  # noqa: E731
    f32 = lambda v: v.astype(np.float32).astype(np.float64)  # noqa: E731
    R = (lambda v: _bf16_round64(f32(v))) if dtype == torch.bfloat16 else f32
    step, m, noise, x1 = f64(step), f64(m), f64(noise), f64(x1)
    tf = float(np.float32(t))              # a Python-float operand enters the fp32 op-math: the double cast to fp32
    omt = float(np.float32(1.0 - t))       # 1 - t in double, then fp32
    a = R(noise * omt)
    b = R(x1 * tf)
    k = R(a + b)
    om = R(1.0 - m)
    out = R(R(step * m) + R(k * om))
    return torch.from_numpy(out).to(torch.float32).to(dtype)


def bits(t):
    """the words of a tensor as integers: the comparison of every word, +-0 told apart"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def operands(n, dtype, seed, mask_kind, device="cpu"):
    """step, mask, noise, x1 of n words in the state dtype: normal draws, with a lane of +-0 and a lane near the top of the bf16 range scaled so
    that no intermediate overflows (|v| <= 2^125: a product with a factor <= 1 and a two-term sum stay below 2^127)"""
    g = torch.Generator().manual_seed(seed)
    step, noise, x1 = (torch.randn(n, generator=g) * s for s in (1.5, 1.0, 1.2))
    for k, v in enumerate((step, noise, x1)):
        v[k::16][: n // 64] = 0.0
        v[k + 3::16][: n // 64] = -0.0
        v[k + 6::16][: n // 64] *= 2.0 ** 123
    if mask_kind == "hard":
        m = (torch.rand(n, generator=g) < 0.5).float()
    elif mask_kind == "eighths":
        m = torch.randint(0, 9, (n,), generator=g).float() / 8
    elif mask_kind == "ones":
        m = torch.ones(n)
    elif mask_kind == "zeros":
        m = torch.zeros(n)
    else:
        assert mask_kind == "soft"
        m = torch.rand(n, generator=g)
    return tuple(v.to(dtype).to(device) for v in (step, m, noise, x1))


def slopes(n, dtype, seed, device="cpu"):
    """y0, k1 .. k4 of n words for the step in front of the blend: normal draws with the same lanes; the slopes' top lane sits at 2^118 so that
    k1 + 3 (k2 + k3) + k4 (at most 8 terms of ~6 sigma) stays far below the top of the range"""
    g = torch.Generator().manual_seed(seed)
    vs = [torch.randn(n, generator=g) * s for s in (1.0, 2.0, 1.5, 1.5, 2.0)]
    for k, v in enumerate(vs):
        v[k::16][: n // 64] = 0.0
        v[k + 3::16][: n // 64] = -0.0
        v[k + 6::16][: n // 64] *= 2.0 ** (120 if k == 0 else 118)
    return tuple(v.to(dtype).to(device) for v in vs)


def step(mode, y0, k1, k2, k3, k4, dt):
    """the closing combine of a step as fixed_grid_odeint writes it; ``dt`` a 0-dim fp32 tensor on the state's device (t1 - t0)"""
    if mode == 0:
        return y0 + dt * k1
    assert mode == 4
    return y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


T_VALUES = (0.0, 0.3, 0.7283, 1.0)  # 0.7283 is neither a bf16 nor an fp32 value
