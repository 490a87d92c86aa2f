"""What one step of the multistep samplers computes (helper of tests/test_multistep_cpu.py and tests/test_gpu_multistep.py; plain module, no
test in here).

``host_step`` is the torch expression of the host loop that defines the feature (transport/multistep.py: ``weight_sum``), on whatever
device the tensors live on: PyTorch's own type promotion and kernels decide every rounding; the weights are Python floats.

``chain64`` restates the same arithmetic without torch's promotion rules: numpy float64, one operation at a time, each result rounded to fp32 (the
op-math format of every elementwise kernel) and then to the state dtype D.  A float64 product of two fp32 operands is exact, a float64 sum of two
is exact or rounds once at 53 bits, which the following rounding to 24 bits hides (53 >= 2 * 24 + 2): every stage is the ONE correct word.

    S(c, k): acc = R(c_0 k_0); acc = R(acc + R(c_j k_j)), j < used(c);   y = R(y_prev + S(a, k));   p = R(y + S(b, k))
"""
import numpy as np
import torch

from lumina_t2x_amd.transport.multistep import used, weight_sum


def host_step(y_prev, ks, a, b, has_corr):
    """(y, p) of one step: ``ks`` newest slope first, ``a`` / ``b`` four Python floats each (fp32 values)"""
    y = weight_sum(y_prev, ks, a) if has_corr else y_prev
    return y, weight_sum(y, ks, b)


def _bf16_round64(x):
    """float64 array holding fp32 values -> the nearest bf16 value (ties to even), by integer arithmetic on the fp32 word"""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).astype(np.float64)


def _rounders(dtype):
    f32 = lambda v: v.astype(np.float32).astype(np.float64)  # noqa: E731
    return (lambda v: _bf16_round64(f32(v))) if dtype == torch.bfloat16 else f32


def _sum64(y, ks, c, R):
    n = used(c)
    if n == 0:
        return y
    acc = R(ks[0] * float(np.float32(c[0])))
    for j in range(1, n):
        acc = R(acc + R(ks[j] * float(np.float32(c[j]))))
    return R(y + acc)


def chain64(y_prev, ks, a, b, has_corr, dtype):
    """(y, p) in float64 with the rounding points stated one by one; operands are tensors of the state dtype; returns tensors of it"""
    f64 = lambda v: v.detach().cpu().to(torch.float64).numpy()  # noqa: E731
    R = _rounders(dtype)
    yp, k = f64(y_prev), [f64(v) for v in ks]
    y = _sum64(yp, k, a, R) if has_corr else yp
    p = _sum64(y, k, b, R)
    back = lambda v: torch.from_numpy(v).to(torch.float32).to(dtype)  # noqa: E731
    return back(y), back(p)


def fused64(y_prev, k0, c0, dtype=torch.float32):
    """``y_prev + c0 * k0`` as a fused multiply-add would give it at an fp32 state: ONE rounding of the exact value"""
    assert dtype == torch.float32
    exact = y_prev.double().numpy() + k0.double().numpy() * float(np.float32(c0))  # exact wherever it is used: see fma_case
    return torch.from_numpy(exact.astype(np.float32))


def bits(t):
    """the words of a tensor as integers: the comparison of every word, +-0 told apart"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# bf16: every weight is 1 + 2^-8 up to sign and a power of two, so its product with a power of two lies exactly half way between two bf16
# values; fp32: 1 + 2^-12 squared is 1 + 2^-11 + 2^-24, half way between two fp32 values
MIDPOINT_WEIGHTS = (1.00390625, -1.00390625, 2.0078125, 0.501953125)
FMA_WEIGHT = 1.000244140625


def operands(n, dtype, seed, device="cpu"):
    """y_prev and four slopes of n words in the state dtype.  Lanes 0 mod 4 hold signed powers of two (with MIDPOINT_WEIGHTS every product of a
    bf16 chain is then a bf16 midpoint: a contracted product, or a missing R, moves the word); lanes 1 mod 4 hold the fp32 fma case (k = 1 + 2^-12,
    y = -(1 + 2^-11): with FMA_WEIGHT as b_0 the separate multiply and add give 0 where a fused one gives 2^-24; at bf16 they are ordinary values);
    the rest are normal draws with +-0 among them."""
    g = torch.Generator().manual_seed(seed)
    vs = [torch.randn(n, generator=g) * s for s in (1.0, 2.0, 1.5, 1.5, 2.0)]
    for k, v in enumerate(vs):
        e = torch.randint(-6, 7, (n,), generator=g).float()
        sgn = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
        v[0::4] = (sgn * torch.exp2(e))[0::4]
        v[1::4] = -(1 + 2.0 ** -11) if k == 0 else 1 + 2.0 ** -12
        v[2::16] = 0.0
        v[3::16] = -0.0
    return tuple(v.to(dtype).to(device) for v in vs)
