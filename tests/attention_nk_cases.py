"""Cases and launches of the per-sample key count tests (plain module, no test in here): tests/test_attention_nk_cpu.py checks the draws
on the CPU, tests/test_gpu_attention_nk.py runs them through lt_op_attention_nk / lt_op_attention_fused_nk.

Operands and expectation are those of tests/exact_attention.py (selector / levels with valid = the per-sample counts, DELTA and
MAX_AMBIGUOUS unchanged).  Before a launch the K rows and V rows (= V^T columns) of every masked key are overwritten with finite words
of magnitude 2^10 and mixed signs: a masked key that leaks - into the maximum, the row sum or O - changes output words by far more than
a rounding, and no score overflows (|q| <= 128, 72 terms: |q . k| < 2^24).  The expectation is computed from the clean draw: it masks the
same keys to -inf, so it never reads those rows."""
import ctypes as C

import torch

import exact_attention as X

HD = 72
# (B, H, Hkv): BH % 8 != 0 takes the plain block mapping; 2 x 8 is GQA (4 query heads per kv-head) on the XCD mapping
SHAPES = [(3, 2, 2), (2, 8, 2)]
# N = Nk = 320: five tiles, the ring of four slots wraps; 256 query rows + a partial block of 64
#   257: one valid key in the fifth tile (a reused slot) | 1: a single-key sample | 191: 63 of 64 valid in the last of three tiles |
#   64: exactly one tile | 256: whole tiles, fewer of them, no mask | 129: three tiles, one valid key in the last | 320 x 3: nk given, nothing masked
COUNTS_320 = [(320, 257, 1), (320, 191, 64), (320, 256, 129), (320, 320, 320)]
# N = Nk = 128: at most two tiles, the mask is written with the constants before the first barrier.  The two lists above at this size:
#   65: one valid key in the second tile | 1 | 127: 63 of 64 valid in the last of two tiles | 64: exactly one tile
COUNTS_128 = [(128, 65, 1), (128, 127, 64)]
FAMILIES = ["selector", "levels"]


def counts_for(B, counts):
    """a batch of two takes the two counts that differ from the layout length"""
    return list(counts) if B == 3 else list(counts[1:])


SELF_CASES = [(B, H, Hkv, N, tuple(counts_for(B, c))) for B, H, Hkv in SHAPES for N, lists in ((320, COUNTS_320), (128, COUNTS_128)) for c in lists]
# fused text phase behind a masked image phase: (B, H, Hkv, N, image counts, Tk, valid text keys)
FUSED_CASES = [(2, 8, 2, 320, (320, 257), 64, (64, 8)), (2, 8, 2, 320, (320, 257), 256, (256, 256))]


def seed_of(N, counts):
    return N + 7 * sum(counts)


def draw(family, B, H, Hkv, N, counts, device="cpu"):
    return X.GENERATORS[family](B, H, Hkv, N, N, HD, seed=seed_of(N, counts), valid=list(counts), device=device)


def fused_draw(family, B, H, Hkv, N, counts, T, tvalid, device="cpu"):
    """exact_attention.fused_draw with per-sample image key counts on the self side"""
    seed = seed_of(N, counts) + T
    a = X.GENERATORS[family](B, H, Hkv, N, N, HD, seed=seed, valid=list(counts), device=device, slot=0, nslots=2)
    t = X.GENERATORS[family](B, H, Hkv, N, T, HD, seed=seed, valid=list(tvalid), device=device, slot=1, nslots=2, kseed=seed + 100)
    a["q"] = t["q"] = (a["q"].float() + t["q"].float()).to(torch.bfloat16)
    return a, t


def poison_masked(inp):
    """(k, v) of the draw with the rows of masked keys replaced by +-1024 / +-1536 (hashed signs and magnitudes)"""
    k, v = inp["k"].clone(), inp["v"].clone()
    B, Hkv, Nk, hd = k.shape
    i = X._ar(Hkv * Nk * hd, k.device).view(Hkv, Nk, hd)
    for b, n in enumerate(inp["valid"]):
        if n < Nk:
            for t, salt in ((k, 21), (v, 22)):
                h = X._mix(i[:, n:] + 1000003 * b, salt)
                t[b, :, n:] = ((1024 + 512 * ((h >> 4) & 1)) * (1 - 2 * (h & 1))).to(t.dtype)
    return k, v


def restricted_use(inp):
    """every_reduction_index_is_used restricted to the valid keys, per sample: the share of (head, whole 64-row block, reduction index)
    triples in which a non-zero q meets a non-zero k of a VALID key"""
    q, k = inp["q"], inp["k"]
    B, H, N, hd = q.shape
    rep = H // k.shape[1]
    shares = []
    for b in range(B):
        kn = (k[b, :, :inp["valid"][b]] != 0).any(1).repeat_interleave(rep, 0)
        qn = (q[b, :, :N // 64 * 64] != 0).view(H, N // 64, 64, hd).any(2)
        shares.append(float((qn & kn[:, None, :]).double().mean()))
    return shares


def describe(B, H, Hkv, N, Nk, hd, has_nk=True, has_text=False, Tkpad=0, bias=False, accumulate=False):
    from gpu_util import lib, ok
    buf = C.create_string_buffer(64)
    ok(lib().lt_op_attention_nk_describe(int(bias), int(accumulate), B, H, Hkv, N, Nk, X.pad64(Nk), hd, int(has_nk), int(has_text), Tkpad, buf, 64))
    return buf.value.decode()


def _nk_dev(counts, device):
    return None if counts is None else torch.tensor(list(counts), dtype=torch.int32, device=device)


def run_nk(q, k, v, counts, out_pair=0, what="", txt=None, gate=None):
    """lt_op_attention_nk (txt None) or lt_op_attention_fused_nk on a guarded NaN-filled output; q / k / v as given (k pre-scaled), counts None:
    nk_dev = NULL.  out_pair: the output is brought back to row-major with lt_op_pair_layout.  -> bf16 [B, H, N, hd]"""
    from exact_operands import Guarded
    from gpu_util import P, lib, ok, stream
    q, k = q.contiguous(), k.contiguous()
    B, H, N, hd = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    Nkpad = X.pad64(Nk)
    vt = X.make_vt(v, Nkpad)
    nk = _nk_dev(counts, q.device)
    guard = Guarded(B * N, H * hd)
    if txt is None:
        ok(lib().lt_op_attention_nk(P(q), P(k), P(vt), None, P(guard.out), None, 0, B, H, Hkv, N, Nk, Nkpad, hd, 1.0, 1, P(nk), int(out_pair), stream()),
           "attention_nk")
    else:
        tk = txt["k"].contiguous()
        T = tk.shape[2]
        Tpad = X.pad64(T)
        tvt, tbias = X.make_vt(txt["v"], Tpad), X.make_bias(txt["valid"], T, Tpad, q.device)
        ok(lib().lt_op_attention_fused_nk(P(q), P(k), P(vt), P(tk), P(tvt), P(tbias), P(gate), P(guard.out), B, H, Hkv, N, Nk, Nkpad, T, Tpad, hd, P(nk),
                                          int(out_pair), stream()), "attention_fused_nk")
    if out_pair:
        ok(lib().lt_op_pair_layout(P(guard.out), B * N, H * hd, 0, stream()), "pair_layout")
    torch.cuda.synchronize()
    guard.assert_intact(what)
    return guard.out.view(B, N, H, hd).permute(0, 2, 1, 3)


def random_operands(B, H, Hkv, N, T, seed, device="cuda"):
    """bf16 operands in the engine's ranges: q, k rows of unit scale per dim (post-LayerNorm), k carrying hd^-1/2 log2(e); v of unit scale"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)  # noqa: E731
    ks = HD ** -0.5 * X.L2E
    q, k, v = rn(B, H, N, HD).to(torch.bfloat16), (rn(B, Hkv, N, HD) * ks).to(torch.bfloat16), rn(B, Hkv, N, HD).to(torch.bfloat16)
    txt = None
    if T:
        txt = dict(k=(rn(B, Hkv, T, HD) * ks).to(torch.bfloat16), v=rn(B, Hkv, T, HD).to(torch.bfloat16), valid=[T] + [8] * (B - 1))
    return q, k, v, txt
