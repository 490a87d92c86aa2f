"""Helper of the tiled-sampling tests (test_tiled_cpu.py, test_gpu_tiled.py): the geometries, operands on which the fusion is exact, the
float64 restatement of ``transport.tiled.fuse`` and its mutants.

Exact operands: ``f`` integer-valued with |f| <= 64 and weights that are powers of two, so every product ``weight * f`` and every partial sum
of at most 64 of them is an integer multiple of 2^-3 below 2^24 - exact in fp32 whatever the order - and so is every weight sum.  The float64
restatement forms the same sums exactly, divides once in float64 and rounds the quotient to fp32, then to the state dtype.  Where the weight sum
is a power of two the division is exact too.  That cannot be arranged for the clamped geometry (lefts 0, 4, 6 put columns 6 and 7 under three
windows and column 10 under two of the same weights: no assignment of powers of two makes every sum one - checked exhaustively over 2^-3 .. 2^3),
so there the sums are 1, 2, 3 and the restatement rests on the division alone: both operands are exact fp32 numbers, fp32 division is correctly
rounded, and rounding a float64 quotient of two fp32 numbers to fp32 equals the correctly rounded fp32 quotient (53 >= 2 * 24 + 2), so the two
agree bit for bit all the same."""
import torch

_COL = (1.0, 1.0, 2.0, 2.0, 1.0, 1.0, 2.0, 2.0)  # w[j] + w[j - 4] is a power of two for j = 4 .. 7


def _w8(rows=False, cols=False):
    r = torch.tensor(_COL if rows else (1.0,) * 8, dtype=torch.float32)
    c = torch.tensor(_COL if cols else (0.5,) * 8, dtype=torch.float32)
    return torch.outer(r, c)


# name -> (canvas_hw, win_hw, offsets, exact weights)
GEOMETRIES = {
    "two_overlap": ((8, 12), (8, 8), [(0, 0), (0, 4)], _w8(cols=True)),
    "four_12x12": ((12, 12), (8, 8), [(0, 0), (0, 4), (4, 0), (4, 4)], _w8(rows=True, cols=True)),  # pixels under 1, 2 and 4 windows
    "clamped_8x14": ((8, 14), (8, 8), [(0, 0), (0, 4), (0, 6)], torch.ones(8, 8)),                   # the last stride is shorter
}
GPU_EXTRA = {"wide_16x24": ((16, 24), (16, 16), [(0, 0), (0, 8)], torch.full((16, 16), 0.25))}


def exact_f(n, C, h, w, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, (n, C, h, w), generator=g).to(dtype)


def random_f(n, C, h, w, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, C, h, w), generator=g).to(dtype)


def cover_counts(offsets, win_hw, canvas_hw):
    cnt = torch.zeros(canvas_hw, dtype=torch.int64)
    for t, l in offsets:
        cnt[t:t + win_hw[0], l:l + win_hw[1]] += 1
    return cnt


def fuse64(f, offsets, weight, canvas_hw, dtype):
    """``fuse`` restated in float64 - exact sums of the products, one division, the quotient rounded to fp32 and then to ``dtype``"""
    n, C, h, w = f.shape
    acc = torch.zeros((C,) + tuple(canvas_hw), dtype=torch.float64)
    ws = torch.zeros(canvas_hw, dtype=torch.float64)
    for k, (t, l) in enumerate(offsets):
        acc[:, t:t + h, l:l + w] += weight.double() * f[k].double()
        ws[t:t + h, l:l + w] += weight.double()
    return (acc / ws).to(torch.float32).to(dtype)


def fuse_mutant(f, offsets, weight, canvas_hw, dtype, mutation):
    """``fuse`` with one thing changed: ``order`` - the windows walked backwards; ``nodiv`` - no division; ``fma`` - the product not rounded
    before the sum (formed exactly in float64, the sum rounded to fp32 once)"""
    n, C, h, w = f.shape
    acc = torch.zeros((C,) + tuple(canvas_hw), dtype=torch.float32)
    ws = torch.zeros(canvas_hw, dtype=torch.float32)
    order = list(enumerate(offsets))
    if mutation == "order":
        order.reverse()
    for k, (t, l) in order:
        sl = acc[:, t:t + h, l:l + w]
        if mutation == "fma":
            acc[:, t:t + h, l:l + w] = (sl.double() + weight.double() * f[k].double()).float()
        else:
            acc[:, t:t + h, l:l + w] = sl + weight * f[k].float()
        ws[t:t + h, l:l + w] = ws[t:t + h, l:l + w] + weight
    return (acc if mutation == "nodiv" else acc / ws).to(dtype)


def words(x):
    """the words of a bf16 / fp32 tensor as integers, -0 mapped to +0"""
    x = x.detach().cpu().contiguous()
    w = x.view(torch.int16).to(torch.int32) & 0xffff if x.dtype == torch.bfloat16 else x.view(torch.int32).to(torch.int64) & 0xffffffff
    neg0 = 0x8000 if x.dtype == torch.bfloat16 else 0x80000000
    return torch.where(w == neg0, torch.zeros_like(w), w)


def toy_model(scales):
    """a ``forward_with_cfg``-shaped torch callable: row r of the input is mapped pointwise with its own 'prompt' ``scales[r]`` and the stage
    time; 2 n rows in, 2 n rows out, every operation in the state dtype"""
    def fn(x, t, **kw):
        s = torch.as_tensor(scales, dtype=x.dtype)[:, None, None, None]
        tt = t.to(x.dtype)[:, None, None, None]
        return torch.tanh(x * s) * (1 + tt) - x * tt
    return fn
