"""The cases and draws of tests/test_gpu_gemm_rounding.py (plain module, no test in here).

Every draw comes from a CPU generator, so tests/test_exact_operands_cpu.py checks the floors of exact_operands.expected_rounded and the
statistic intervals on the very operands the GPU file runs; the GPU file moves them to the device and computes the same expected words
there (the preconditions are asserted again on every call).  Shapes: the smallest with a whole tile, a ragged edge in M and N and two K
slabs - or, where the launch needs one tile per CU (fused QKV, pair layout, the statistics of the persistent kernel), the smallest
with 256 tiles at K = 192."""
import functools

import torch

import exact_operands as X

PLAIN_SHAPES = [(300, 576, 128), (259, 296, 192)]   # (the ragged corner fragment keeps 3 x 8 words: every fragment must hold an inexact one)
LONG_K_SHAPE = (300, 576, 2304)
PLAIN_CASES = ([(*s, v, bd) for s in PLAIN_SHAPES for v in (1, 2, 3, 7, 8) for bd in (None, 0, 1)] + [(*s, v, None) for s in PLAIN_SHAPES for v in (15, 16)] +
               [(*LONG_K_SHAPE, v, None) for v in (1, 3, 15)])   # K >= 2048 once on the classic, the ping-pong and the persistent kernel
SWIGLU_SHAPES = [(300, 576, 192), (257, 320, 128)]               # M x N = 2 F x K
SWIGLU_CASES = [(*s, v) for s in SWIGLU_SHAPES for v in (1, 3, 7, 15)]
VT_CASES = [(64, 3, 2, 72, 128, 1), (64, 3, 2, 72, 128, 2), (128, 2, 8, 72, 576, 1), (128, 2, 8, 72, 576, 2)]   # tokens, B, kv heads, head_dim, K, variant
QKV_CASES = [(320, 16, 16, 16, 96, 256), (320, 24, 16, 16, 72, 192)]   # the two smallest rows of test_gpu_gemm_exact.QKV_SHAPES: 256- and 288-wide tiles
PAIR_CASES = [(7424, 2304, 192, 0, 0), (4096, 4096, 192, 1, 0), (4096, 4096, 192, 1, 1)]   # M, N, K, epilogue, pair_c: 261 / 256 tiles of 256 x 256
SPLITK_CASES = [  # M, N, K, entry point, parts the launch must take: rows of test_gpu_gemm_exact.SPLITK_CASES and two ragged ones
    (512, 1536, 1536, "splitk", 2), (500, 1528, 1024, "splitk", 2), (512, 1536, 768, "splitk", 0), (512, 1536, 1536, "auto", 2),
    (512, 1536, 4096, "auto", 4), (500, 1528, 4096, "auto", 4), (512, 1536, 768, "auto", 0)]
GROUPED = dict(E=6, K=256, N=384, te=[2, 0, -1, 3, 5, 1, 4, 4])
GROUPED_GATHER = dict(E=5, K=256, N=320, T=600, te=[2, 2, 0, -1, 3, 1, 4, -1], fill={0: 256, 1: 256, 2: 200, 4: 131, 5: 256, 6: 97})
GROUPED_TAIL = dict(K=512, N=256, ntile=300, holes=5)            # 295 valid tiles: one round of 256 CUs and a tail of 39
YSTAT = dict(B=2, N=3712, d=2304, K=192)                         # 29 x 9 tiles of 256 x 256: the smallest y the persistent kernel takes at d = 2304
QSTAT = dict(B=24, tokens=320, H=16, Hkv=16, hd=72, K=192, grid_w=16)
ROWSTAT = dict(B=2, tokens=64, H=8, Hkv=8, hd=48, K=384, grid_w=8)
TOP_SHAPE = (300, 296, 192)
TOP_VARIANTS = (1, 2, 3, 7, 8, 15, 16)
FILL = 3.0


def gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator().manual_seed(seed % (1 << 62))


@functools.lru_cache(maxsize=2)
def plain_problem(M, N, K, bias_dtype, device):
    """(A, W, bias, want, shares) on `device`"""
    A, W, b = X.rounded_operands(M, N, K, gen(M, N, K, -1 if bias_dtype is None else bias_dtype), bias_dtype)
    A, W, b = A.to(device), W.to(device), None if b is None else b.to(device)
    info = {}
    return A, W, b, X.expected_rounded(A, W, b, info=info), info


@functools.lru_cache(maxsize=2)
def swiglu_problem(M, F_, K, device):
    """(A, w1, w3, want, keep, shares)"""
    A, w1, w3 = (t.to(device) for t in X.swiglu_rounded_operands(M, F_, K, gen(M, F_, K, 13)))
    info = {}
    want, keep = X.swiglu_expected_rounded(A, w1, w3, info=info)
    return A, w1, w3, want, keep, info


@functools.lru_cache(maxsize=1)
def top_problem(device):
    """(A, W, want): sums up to 2046 2^117 of either sign; the draw's own conditions instead of the generator's floors"""
    A, W = X.top_of_range_operands(*TOP_SHAPE[:2], TOP_SHAPE[2], device)
    want = X.expected_rounded(A, W, floors=None)
    n = (A.double() @ W.double().t()).abs() / 2.0 ** 117
    w = want.float()
    if not (bool(torch.isfinite(n).all()) and float(n.max()) < 2048):
        raise X.PreconditionError("an exact sum reaches 2^128")
    below, above = (n > 2040) & (n < 2044), n >= 2044
    for sign in (1, -1):
        rows = (w.sign() == sign)
        if int((below & rows).sum()) < 256 or int((above & rows).sum()) < 256 or int(((n == 2044) & rows).sum()) < 16:
            raise X.PreconditionError("too few sums between the largest finite bf16 and 2^128")
    if not (bool((w.abs()[below] == X.BF16_MAX).all()) and bool(torch.isinf(w[above]).all()) and bool(torch.isfinite(w[~above]).all())):
        raise X.PreconditionError("the expected words at the top of the range are not (largest finite | inf)")
    return A, W, want


def expert_weights(E, N, K, epilogue, g):
    """[E, N, K] as the kernel reads it (SwiGLU: packed w1 | w3) and the per-expert halves; every expert its own matrix"""
    if epilogue:
        w1 = (X.sparse_ints((E, N // 2, K), X.SWIGLU_W1_DENSITY, g, X.SWIGLU_W1_AMP) * 2.0 ** X.SWIGLU_W1_EXP).to(torch.bfloat16)
        w3 = X.sparse_ints((E, N // 2, K), X.DENSITY_W, g, X.AMP_W).to(torch.bfloat16)
        return torch.stack([X.pack_w13_ref(w1[e], w3[e]) for e in range(E)]).contiguous(), (w1, w3)
    return torch.stack([X.scale_w(X.sparse_ints((N, K), X.DENSITY_W, g, X.AMP_W)) for _ in range(E)]).to(torch.bfloat16).contiguous(), None


def grouped_a(rows, K, epilogue, g):
    A = X.sparse_ints((rows, K), X.DENSITY_A, g, X.amp_a(K))
    return (A if epilogue else X.scale_a(A)).to(torch.bfloat16)


def grouped_expected(A, W, halves, te, epilogue, info=None):
    """[M, N or N / 2] (and the keep mask): rows of tile t times the matrix of expert te[t]; padding segments keep FILL"""
    M, No = A.shape[0], W.shape[1] // 2 if epilogue else W.shape[1]
    want = torch.full((M, No), FILL, device=A.device, dtype=torch.bfloat16)
    keep = torch.ones((M, No), device=A.device, dtype=torch.bool)
    tile = torch.tensor(te, device=A.device).repeat_interleave(256)
    for e in sorted(set(x for x in te if x >= 0)):
        rows = tile == e
        if epilogue:
            want[rows], keep[rows] = X.swiglu_expected_rounded(A[rows], halves[0][e].to(A.device), halves[1][e].to(A.device), info=info)
        else:
            want[rows] = X.expected_rounded(A[rows], W[e], info=info)
    return want, keep


@functools.lru_cache(maxsize=2)
def grouped_problem(epilogue, device):
    c = GROUPED
    g = gen(17, epilogue)
    A = grouped_a(256 * len(c["te"]), c["K"], epilogue, g).to(device)
    W, halves = expert_weights(c["E"], c["N"], c["K"], epilogue, g)
    W = W.to(device)
    info = {}
    want, keep = grouped_expected(A, W, halves, c["te"], epilogue, info)
    return A, W, want, keep, info


def stat_problem(M, N, K, width, which, device, q_cols=None):
    """(A, W, want, value, bound, shares): a plain draw and the slot statistics of its first q_cols expected rounded words"""
    A, W, _, want, info = plain_problem(M, N, K, None, device)
    info = dict(info)
    q = N if q_cols is None else q_cols
    value, bound = X.expected_slot_stats(want[:, :q], A.double() @ W[:q].double().t(), width, f"{M}x{N}x{K} slots of {width}", which, info)
    return A, W, want, value, bound, info
