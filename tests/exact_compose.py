"""Helpers of the composed-guidance tests: operands on which every intermediate of ``guided_compose``'s chain is exact, a float64
restatement of the chain, a restatement with explicit rounding points that three mutants are cut from, and word-level comparison.

Exact operands.  Model outputs are integers in [-2, 2] (bf16 values in either io dtype) and weights are +-0.5, +-1, +-2.  Then ``c_k - u`` is an
integer in [-4, 4], ``w_k (c_k - u)`` a multiple of 0.5 of magnitude <= 8, a partial sum of up to 7 such terms a multiple of 0.5 of magnitude
<= 56 and ``u + acc`` one of magnitude <= 58: at most 116 half-units, which the 8 significant bits of bf16 hold.  No rounding point rounds,
so float64 arithmetic without any rounding gives the same words - ``compose64`` asserts that every R it applies is the identity."""
import torch

POW2 = (0.5, 1.0, 2.0, -0.5, -1.0, -2.0)


def words(x, fold_zero=False):
    """the words of a bf16 / fp32 tensor as integers; ``fold_zero``: -0 mapped to +0"""
    x = x.detach().cpu().contiguous()
    w = x.view(torch.int16).to(torch.int32) & 0xffff if x.dtype == torch.bfloat16 else x.view(torch.int32).to(torch.int64) & 0xffffffff
    if fold_zero:
        neg0 = 0x8000 if x.dtype == torch.bfloat16 else 0x80000000
        w = torch.where(w == neg0, torch.zeros_like(w), w)
    return w


def exact_outs(K, Bp, C, H, W, dtype, seed=0):
    """integer-valued model outputs ``[(K + 1) Bp, C, H, W]`` in [-2, 2] and K power-of-two weights"""
    g = torch.Generator().manual_seed(seed)
    outs = torch.randint(-2, 3, ((K + 1) * Bp, C, H, W), generator=g).to(dtype)
    idx = torch.randint(0, len(POW2), (K,), generator=g).tolist()
    return outs, [POW2[i] for i in idx]


def random_outs(K, Bp, C, H, W, dtype, seed=0):
    """random bf16 values (held in ``dtype``) and weights that are no powers of two"""
    g = torch.Generator().manual_seed(seed)
    outs = (3.0 * torch.randn((K + 1) * Bp, C, H, W, generator=g)).to(torch.bfloat16).to(dtype)
    w = (torch.rand(K, generator=g) * 6.0 - 2.0).tolist()
    return outs, [float(torch.tensor(v, dtype=torch.float32)) for v in w]


def _r64(v, exact):
    r = v.to(torch.float32).to(torch.bfloat16).to(torch.float64)
    if exact:
        assert torch.equal(r, v), "an intermediate of the chain is not exact on these operands"
    return r


def compose64(outs, weights, ch, exact=True):
    """the chain of the issue word for word, in float64: acc = R(w_1 R(c_1 - u)); acc = R(acc + R(w_k R(c_k - u))), k = 2 .. K; g = R(u + acc)"""
    K = len(weights)
    rows = outs.to(torch.float64).chunk(K + 1)
    u = rows[K][:, :ch]
    acc = _r64(weights[0] * _r64(rows[0][:, :ch] - u, exact), exact)
    for k in range(1, K):
        acc = _r64(acc + _r64(weights[k] * _r64(rows[k][:, :ch] - u, exact), exact), exact)
    g = _r64(u + acc, exact)
    return torch.cat([g, rows[0][:, ch:]], 1).to(outs.dtype)


def _r(v):
    return v.to(torch.bfloat16).to(torch.float32)


def compose_stated(outs, weights, ch, *, reverse=False, drop_inner=False, base_from_last=False):
    """the chain with its rounding points written out on fp32 tensors (each fp32 operation rounds to fp32, then R to bf16: what a bf16 tensor
    operation does).  Unmutated it equals ``guided_compose``; the three mutants: the sum taken from prompt K down to prompt 1, the rounding of
    ``w_k (c_k - u)`` dropped before it is added, the base row taken from prompt K."""
    K = len(weights)
    rows = outs.to(torch.float32).chunk(K + 1)
    u = (rows[K - 1] if base_from_last else rows[K])[:, :ch]
    w = [torch.tensor(v, dtype=torch.float32) for v in weights]
    order = list(reversed(range(K))) if reverse else list(range(K))
    inner = (lambda v: v) if drop_inner else _r
    k0 = order[0]
    acc = _r(w[k0] * _r(rows[k0][:, :ch] - u))
    for k in order[1:]:
        acc = _r(acc + inner(w[k] * _r(rows[k][:, :ch] - u)))
    g = _r(u + acc)
    return torch.cat([g, rows[0][:, ch:]], 1).to(outs.dtype)
