"""Float64 restatement of the query blur of smoothed-energy guidance (csrc/query_blur.hip), for test_seg_cpu.py / test_gpu_seg.py.

q is [B, H, N = Hp * grid_w, hd]; columns 0 .. blur_w - 1 of a grid row are image tokens, the others (Flag-DiT's end-of-line token) pass through
and are nobody's neighbour.  `blur_ref` is the separable form (horizontal, then vertical, reflection without repeating the edge), `blur_matrix`
the explicit dense N x N matrix of the same map, `mean_ref` mode 1.  `blur_bound` is the absolute fp32-accumulation bound of the kernel's two
chains of 2 r + 1 fused multiply-adds (derived in DESIGN 7t):  |got - exact| <= gamma_{2 (2 r + 1)} * blur(|q|),  gamma_n = n u / (1 - n u),
u = 2^-24.  `check_words` holds a kernel's words to RN_bf16(ref), the other neighbour only where ref lies within that bound of a bf16 midpoint."""
import torch

from exact_attention import neighbours


def refl(i, n):
    return -i if i < 0 else 2 * (n - 1) - i if i >= n else i


def clamp(i, n):
    """the WRONG boundary rule (the edge repeated), for the chain mutation 'no reflection'"""
    return min(max(i, 0), n - 1)


def _pass(x, taps, axis, n, edge=refl):
    """sum_k taps[k] * x[edge(i + k - r)] along `axis` (length n), float64"""
    r = (len(taps) - 1) // 2
    assert r <= n - 1, (r, n)
    out = torch.zeros_like(x)
    for k in range(-r, r + 1):
        idx = torch.tensor([edge(i + k, n) for i in range(n)])
        out = out + float(taps[k + r]) * x.index_select(axis, idx)
    return out


def blur_ref(q, grid_w, blur_w, taps, edge=refl):
    """q: [B, H, N, hd] (any float dtype) -> float64 [B, H, N, hd], unrounded"""
    B, H, N, hd = q.shape
    Hp = N // grid_w
    x = q.double().view(B, H, Hp, grid_w, hd)
    img = _pass(_pass(x[:, :, :, :blur_w], taps, 3, blur_w, edge), taps, 2, Hp, edge)
    return torch.cat([img, x[:, :, :, blur_w:]], 3).reshape(B, H, N, hd)


def blur_matrix(Hp, grid_w, blur_w, taps):
    """the dense [N, N] float64 matrix: out[n] = sum_m M[n, m] q[m]"""
    r = (len(taps) - 1) // 2
    N = Hp * grid_w
    M = torch.zeros(N, N, dtype=torch.float64)
    for y in range(Hp):
        for x in range(grid_w):
            n = y * grid_w + x
            if x >= blur_w:
                M[n, n] = 1.0
                continue
            for ky in range(-r, r + 1):
                for kx in range(-r, r + 1):
                    M[n, refl(y + ky, Hp) * grid_w + refl(x + kx, blur_w)] += float(taps[ky + r]) * float(taps[kx + r])
    return M


def mean_ref(q, grid_w, blur_w):
    B, H, N, hd = q.shape
    Hp = N // grid_w
    x = q.double().view(B, H, Hp, grid_w, hd).clone()
    m = x[:, :, :, :blur_w].sum((2, 3), keepdim=True) / float(Hp * blur_w)
    x[:, :, :, :blur_w] = m
    return x.reshape(B, H, N, hd)


def rn_bf16(x64):
    return neighbours(x64, 0.0)[0]


def blur_bound(q, grid_w, blur_w, taps):
    """absolute error bound of the kernel's fp32 accumulation per word (0 on the pass-through tokens)"""
    n = 2 * len(taps)
    u = 2.0 ** -24
    b = blur_ref(q.double().abs(), grid_w, blur_w, taps) * (n * u / (1 - n * u))
    B, H, N, hd = q.shape
    b = b.view(B, H, N // grid_w, grid_w, hd)
    b[:, :, :, blur_w:] = 0.0
    return b.reshape(B, H, N, hd)


def check_words(got, ref, bound, what):
    """got: bf16; ref, bound: float64.  -> share of the words that needed the allowance.  The rule is exact_rows.py's single-rounding form: a
    word lies in RN(ref - bound) .. RN(ref + bound).  Off the midpoints that is RN(ref) alone; within `bound` of a midpoint it is the two
    neighbours; and it is more than two words only where the taps' terms cancel to a value whose bf16 ulp is below the bound (a blur of
    zero-mean queries at a large radius: |ref| < 2^8 bound), where no fp32 accumulation can promise a neighbour."""
    rn = neighbours(ref, 0.0)[0]
    g = got.float().cpu()
    exact = g == rn
    ok = exact | ((g >= neighbours(ref - bound, 0.0)[0]) & (g <= neighbours(ref + bound, 0.0)[0]))
    _, lo, hi, _ = neighbours(ref, 0.0)
    wide = int((ok & (g != lo) & (g != hi)).sum())      # words beyond the two neighbours of ref: the cancelled ones only
    assert wide <= max(2, g.numel() // 10000), f"{what}: {wide} of {g.numel()} words lie beyond the two bf16 neighbours of the reference"
    bad = int((~ok).sum())
    assert bad == 0, f"{what}: {bad} of {g.numel()} words wrong ({int(torch.isnan(g).sum())} NaN); first at {(~ok).nonzero()[0].tolist()}"
    return float((~exact).sum()) / g.numel()
