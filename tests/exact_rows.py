"""Row-kernel checks (csrc/norm.hip, csrc/qkv_post.hip): float64 restatements that follow the kernels' rounding points stage by stage, the
word-exact comparator, and fp32 emulations of the same chains for the CPU tests (plain module, no test in here).

Every kernel is a chain  statistic -> rounding -> exact product -> rounding -> ...  (norm.hip's header comments, apply_rms_mod_store):
  * the statistic (rinv, mean, rstd) is computed here in float64 from the bf16 inputs; the kernel's fp32 value differs from it by at most
    a relative DELTA (below), which is the only inexact input of the chain;
  * a bf16 x bf16 product is exact in fp32 (16 significant bits), so a stage `bfr(c * w)` has ONE correct word once c is fixed; a sum of two
    bf16 values carries at most one fp32 rounding (U = 2^-24 relative) in front of its bf16 rounding;
  * (the single-rounding LayerNorm forms accept RN(p - bound) .. RN(p + bound), which is the same two neighbours except on the rare word
    whose terms cancel below the bound itself)
  * at each rounding stage a value whose float64 pre-image lies within the stage's ABSOLUTE error bound of a bf16 midpoint is ambiguous:
    both neighbours are carried forward through the remaining stages (exact_attention.neighbours with a per-word delta); a word of the
    output is accepted only if it equals one candidate.  The share of ambiguous words is capped per call (MAX_AMBIGUOUS), as a condition
    on the inputs: PreconditionError, never a looser comparison.
  * the LayerNorm forms (LayerNorm -> affine -> RoPE -> out_scale in qkv_post.hip; final LayerNorm -> modulate in norm.hip) round ONCE; their
    bound is absolute per word and built from the magnitudes of the terms, so that the cancellation in `x - mean` (the fp32 mean errs by a
    multiple of U mean|x| also where the mean itself is tiny) and in `a cos - b sin` is covered.
  * where a later statistic depends on an output that is itself checked (x' of gated_residual_norm feeds the next norm; h feeds the router),
    the later chain starts from the words the kernel WROTE, after they passed their own comparison.

DELTA, derived from the fp32 operation counts (U = 2^-24; worst case, every rounding in the same direction; positive terms):
  RMS statistic, d <= 4096: per lane 8 elements x MAXCH <= 8 chunks in four v_dot2 accumulators (2 roundings per step: 16), their tree (2),
    the wave butterfly (6), / d and + eps (2): 26 U on the sum, 13 U on its rsqrt; v_rsq_f32 is documented as 1 ulp (2 U); the product
    x * rinv 1 U: 16 U = 2^-20.  The streaming kernel's slot sum (<= 18 slots, pairs: 10) and its four-accumulator second norm stay below.
    apex order (x * rinv * w in fp32): one more product, 17 U.
  LayerNorm, MAXCH chunks: mean: 4 MAXCH serial adds per lane component + 1 + 6 + 1 -> an ABSOLUTE (4 MAXCH + 8) U mean|x|; rstd: half of
    (4 MAXCH + 7 + 4) U plus 2 U, relative; the subtraction and every product 1 U relative to their own result; the RoPE sum 2 U relative to
    |a cos| + |b sin|.  The per-word bound is assembled from these term by term (ref_qk_norm_rope, ref_gated_h).
  qstat: wave butterfly over <= 64 partials (6), 1 / width and the product (2): 8 U on sum / width and on E[x^2]; var = E[x^2] - mean^2.
  tanh (lt_op_prep_mod) and exp / reciprocal of the router weights: the device library's documented bounds (tanh <= 5 ulp, the OpenCL
    full-profile figure the ROCm device libraries are built to; native exp2 / rcp 1 ulp): 10 U and 8 U.
The hardware rsqrt / tanh accuracy has NOT been measured by this project: the ISA's / library's documented bound is used; words outside it
on the GPU are a finding.  The CPU tests measure the fp32 emulations' statistic in three summation orders (the kernel's, serial, torch's
pairwise) against float64: the larger of derived and measured, times a margin of 4, is the DELTA below (test_exact_rows_cpu.py asserts
that the measured figures stay below the derived ones)."""
import math

import torch

from exact_attention import MAX_AMBIGUOUS, neighbours
from exact_operands import PreconditionError, _runs

U = 2.0 ** -24
MARGIN = 4.0
RMS_DERIVED, APEX_DERIVED = 16 * U, 17 * U
DELTA_RMS, DELTA_APEX = MARGIN * RMS_DERIVED, MARGIN * APEX_DERIVED       # 2^-18, 1.06 * 2^-18
DELTA_SUM = U                                                             # one fp32 rounding of a two-term sum (not a statistic: no margin)
DELTA_TANH, DELTA_ROUTE_W = MARGIN * 10 * U, MARGIN * 8 * U
QSTAT_SUM = MARGIN * 8 * U
LT_MOE_MAX_E = 8
GUARD = 7.0


def maxch(d):
    n = ((d >> 3) + 63) // 64
    return 8 if n >= 7 else n


def ln_derived(width):
    """(mean error over mean|x|, relative rstd error) of the LayerNorm statistic, unmargined"""
    m = maxch(width)
    return (4 * m + 8) * U, (2 * m + 7.5) * U


def ln_bounds(width):
    c_mean, c_rstd = ln_derived(width)
    return MARGIN * c_mean, MARGIN * c_rstd, MARGIN * U


def route_logit_delta(d):
    """fp32 dot of a row with a router row: 8 MAXCH serial multiply-adds per lane (2 roundings each), the butterfly (6)"""
    return MARGIN * (16 * maxch(d) + 6) * U


def f32(v):
    """the float32 value of a Python float, as a Python float (eps, out_scale and the watershed cross the C ABI as float)"""
    return float(torch.tensor(v, dtype=torch.float32))


def d64(t):
    return None if t is None else t.detach().to("cpu").double()


def rn(p):
    """round-to-nearest-even bf16 of float64 values, as float64"""
    return neighbours(p, 0.0)[0].double()


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
class Chain:
    """candidates of one output tensor through its rounding stages"""

    def __init__(self, shape):
        self.cands = [None]
        self.amb = torch.zeros(shape, dtype=torch.bool)
        self.first = None          # float64 pre-image of the last stage on the round-to-nearest path (for messages)

    def round(self, f, err=None, rel=None, sum2=False):
        """one rounding stage: f(previous candidate) -> float64 pre-image; err: absolute bound per word (tensor), rel: relative bound;
        neither: the pre-image is exact in fp32, one correct word.  sum2: the pre-image is the sum of two bf16 values - where fp32 holds it
        exactly (ties included: they round to even) there is one correct word, elsewhere one fp32 rounding precedes the bf16 one"""
        if sum2:
            rel = DELTA_SUM
        new = []
        for i, c in enumerate(self.cands):
            p = f(c)
            if i == 0:
                self.first = p
            if err is None and rel is None:
                new.append(rn(p))
                continue
            delta = torch.full_like(p, rel) if err is None else err / p.abs().clamp_min(1e-300)
            r, lo, hi, amb = neighbours(p, delta)
            if sum2:
                amb &= p.float().double() != p
            self.amb |= amb
            new.append(torch.where(amb, lo, r).double())
            if bool(amb.any()):
                new.append(torch.where(amb, hi, r).double())
        self.cands = new
        return self

    def round_once(self, p, err):
        """the single rounding of the LayerNorm forms: every word RN(v) with v in [p - err, p + err] is admissible - rounding is monotonic, so
        that is the range RN(p - err) .. RN(p + err): one word off the midpoints, the two neighbours near one, and more only where the terms
        cancel so far that the bound exceeds the word's own spacing.  Ambiguous: every word with more than one admissible value"""
        self.first, self.cands = p, None
        self.lo, self.hi = rn(p - err), rn(p + err)
        self.amb |= self.lo != self.hi
        return self

    @property
    def want(self):
        return rn(self.first)


def _per_row(v, B, N):
    """[B, d] per-sample vector -> [B * N, d]"""
    return None if v is None else v.repeat_interleave(N, dim=0)


def rms_rinv(x, eps):
    return torch.rsqrt((x * x).mean(-1, keepdim=True) + f32(eps))


def _one_plus(scale, scale_pre):
    return scale if scale_pre else rn(1.0 + scale)    # (1 + bf16 is exact in fp32 unless |scale| < 2^-16, where the word is 1 either way)


def chain_rms_mod(x, rinv, w, scale1, shift, apex=0, ch=None):
    """apply_rms_mod_store: bfr(bfr(bfr(x rinv) w) s1) + shift, each step optional; scale1: bf16(1 + scale) per row or None"""
    ch = ch or Chain(x.shape)
    if w is not None and apex:
        ch.round(lambda _: x * rinv * w, rel=DELTA_APEX)
    else:
        ch.round(lambda _: x * rinv, rel=DELTA_RMS)
        if w is not None:
            ch.round(lambda c: c * w)
    if scale1 is not None:
        ch.round(lambda c: c * scale1)
    if shift is not None:
        ch.round(lambda c: c + shift, sum2=True)
    return ch


def ref_rmsnorm_mod(x, w, scale, shift, B, N, eps, scale_pre=0, apex=0):
    x, w, scale, shift = d64(x), d64(w), _per_row(d64(scale), B, N), _per_row(d64(shift), B, N)
    s1 = None if scale is None else _one_plus(scale, scale_pre)
    return chain_rms_mod(x, rms_rinv(x, eps), w, s1, shift, apex)


def moe_combine(ys, pos, wts):
    """y[row] = bfr(bfr(0 + bfr(w_a ys[pos_a])) + bfr(w_b ys[pos_b])): products exact; the sum of two bf16 values is exact in fp32 unless
    they lie 2^16 apart - a draw on which a combined word is ambiguous is refused (the first statistic depends on every word of y)"""
    ys, wts, pos = d64(ys), d64(wts), pos.cpu().long()
    a, b = rn(wts[:, 0:1] * ys[pos[:, 0]]), rn(wts[:, 1:2] * ys[pos[:, 1]])
    ch = Chain(a.shape).round(lambda _: a + b, sum2=True)
    if bool(ch.amb.any()):
        raise PreconditionError("MoE combine: a combined word lies within one fp32 rounding of a bf16 midpoint")
    return ch.cands[0]


def ref_gated_x(x, y, post_w, gate, B, N, eps, post_mode=1, apex=0, ystat=None):
    """x' = bfr(x + bfr(g bfr(bfr(y rinv) w))) with the prepared gate (gate_mode 0; gate None: gate_mode 2); ystat: [rows, slots] partial sums
    of squares the streaming kernel reads instead of reducing y (summed here in float64)"""
    x, y, post_w, gate = d64(x), d64(y), d64(post_w), _per_row(d64(gate), B, N)
    ch = Chain(x.shape)
    if post_mode == 1:
        if ystat is not None:
            rinv = torch.rsqrt(d64(ystat).sum(-1, keepdim=True) / x.shape[1] + f32(eps))
        else:
            rinv = rms_rinv(y, eps)
        if apex:
            ch.round(lambda _: y * rinv * post_w, rel=DELTA_APEX)
        else:
            ch.round(lambda _: y * rinv, rel=DELTA_RMS).round(lambda c: c * post_w)
        if gate is not None:
            ch.round(lambda c: gate * c)
    elif gate is not None:
        ch.round(lambda _: gate * y)
    else:
        ch.cands = [y]
    ch.round(lambda c: x + c, sum2=True)
    return ch


def ln_stats(x, eps):
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + f32(eps))
    return mean, rstd, x.abs().mean(-1, keepdim=True)


def ref_gated_h(xn, next_w, next_scale, next_shift, B, N, eps, eps_next, next_mode, scale_pre=1, apex=0):
    """h from the x' words the kernel wrote: next_mode 1 the next pre-norm + modulate, 2 the final affine-free LayerNorm + modulate"""
    xn, next_w = d64(xn), d64(next_w)
    scale, shift = _per_row(d64(next_scale), B, N), _per_row(d64(next_shift), B, N)
    s1 = None if scale is None else _one_plus(scale, scale_pre)
    if next_mode == 1:
        return chain_rms_mod(xn, rms_rinv(xn, eps), next_w, s1, shift, apex)
    mean, rstd, mabs = ln_stats(xn, eps_next)
    cm, cr, u = ln_bounds(xn.shape[1])
    p = (xn - mean) * rstd
    e = cm * mabs * rstd + (cr + 2 * u) * p.abs()          # the mean's error; rstd's, the subtraction and the product relative to the value
    if s1 is not None:
        p = p * s1
        e = e * s1.abs() + u * p.abs()
    if shift is not None:
        p = p + shift
        e = e + u * p.abs()
    return Chain(xn.shape).round_once(p, e)


# ---- q / k post-processing --------------------------------------------------------------------------------------------------------------
def rope_table(cs_len, nfreq, theta=10000.0, scales=(0.5, 1.0), ntk=(1.0, 2.0)):
    """[2][cs_len][nfreq][2] (cos, sin) in fp32, built in float64: branch 0 positions scaled (linear interpolation), branch 1 theta scaled
    (NTK).  The kernel and the reference read exactly these factors."""
    out = torch.empty(2, cs_len, nfreq, 2, dtype=torch.float64)
    pos = torch.arange(cs_len, dtype=torch.float64)[:, None]
    for br in range(2):
        freq = 1.0 / ((theta * ntk[br]) ** (torch.arange(nfreq, dtype=torch.float64) / nfreq))[None, :]
        ang = pos * scales[br] * freq
        out[br, ..., 0], out[br, ..., 1] = torch.cos(ang), torch.sin(ang)
    return out.float()


def rope_factors(table, branch, B, N, hd, rope_mode, grid_w, n_tok_b=None, grid_w_b=None, fault=None):
    """(cos, sin) float64 [B * N, hd / 2] per complex slot: model.py:915-963 as qkv_post.hip states it"""
    nslot = hd // 2
    n = torch.arange(N)
    cos, sin = torch.empty(B, N, nslot, dtype=torch.float64), torch.empty(B, N, nslot, dtype=torch.float64)
    pr = torch.arange(nslot)
    for b in range(B):
        n_rot = n.clamp(max=int(n_tok_b[b]) - 1) if n_tok_b is not None and fault != "pad_own_index" else n
        if rope_mode == 1:
            gw = int(grid_w_b[b]) if grid_w_b is not None else grid_w
            gr, gc = n_rot // gw, n_rot % gw
            odd = (pr & 1).bool()[None, :]
            if fault == "swap_row_col":          # one complex slot (slot 1) rotates with the row instead of the column position
                odd = odd.clone()
                odd[:, 1] = False
            pos = torch.where(odd, gc[:, None], gr[:, None])
            fi = (pr >> 1)[None, :].expand(N, nslot)
        else:
            pos, fi = n_rot[:, None].expand(N, nslot), pr[None, :].expand(N, nslot)
        t = table[branch].double()[pos, fi]
        cos[b], sin[b] = t[..., 0], t[..., 1]
    return cos.view(B * N, nslot), sin.view(B * N, nslot)


def ref_qk_norm_rope(src, col0, ln_w, ln_b, ln_eps, B, N, heads, hd, rope_mode, table, branch, grid_w, out_scale=1.0, n_tok_b=None,
                     grid_w_b=None):
    """Chain over the logical [B * N, heads * hd] image (head_major() maps the kernel's [B, heads, N, hd] output onto it)"""
    width = heads * hd
    x = d64(src)[:, col0:col0 + width]
    ln_w, ln_b = d64(ln_w), d64(ln_b)
    cm, cr, u = ln_bounds(width)
    if ln_w is not None:
        mean, rstd, mabs = ln_stats(x, ln_eps)
        t = (x - mean) * rstd * ln_w
        a = t + ln_b
        e = cm * mabs * rstd * ln_w.abs() + (cr + 3 * u) * t.abs() + u * a.abs()
    else:
        a, e = x, torch.zeros_like(x)
    exact = ln_w is None and rope_mode == 0 and out_scale == 1.0
    if rope_mode != 0:
        cos, sin = rope_factors(table, branch, B, N, hd, rope_mode, grid_w, n_tok_b, grid_w_b)
        cos, sin = cos[:, None, :], sin[:, None, :]
        a4, e4 = a.view(B * N, heads, hd // 2, 2), e.view(B * N, heads, hd // 2, 2)
        a0, a1, e0, e1 = a4[..., 0], a4[..., 1], e4[..., 0], e4[..., 1]
        a = torch.stack([a0 * cos - a1 * sin, a0 * sin + a1 * cos], -1).view(B * N, width)
        # the errors of a, two product roundings and the sum's: relative to the MAGNITUDES of the two terms (they may cancel)
        ident = ((sin == 0) & (cos == 1)).expand_as(a0)      # position 0: the rotation multiplies by 1 and 0 and adds 0, exact in fp32
        e = torch.stack([torch.where(ident, e0, e0 * cos.abs() + e1 * sin.abs() + 2 * u * ((a0 * cos).abs() + (a1 * sin).abs())),
                         torch.where(ident, e1, e0 * sin.abs() + e1 * cos.abs() + 2 * u * ((a0 * sin).abs() + (a1 * cos).abs()))], -1).view(B * N, width)
    osc = f32(out_scale)
    if osc != 1.0:
        a = a * osc
        # (an exactly known factor times an out_scale of a few bits - 0.1875 - is exact in fp32: no rounding to allow for, and a tie rounds to even)
        e = e * abs(osc) + torch.where((e == 0) & (a.float().double() == a), torch.zeros_like(a), u * a.abs())
    ch = Chain(a.shape)
    return ch.round(lambda _: a) if exact else ch.round_once(a, e)


def head_major(dst, B, N, heads, hd):
    """the kernel's [B, heads, N, hd] -> logical [B * N, heads * hd]"""
    return dst.view(B, heads, N, hd).permute(0, 2, 1, 3).reshape(B * N, heads * hd)


def from_pair(buf, rows, d):
    """row-pair-interleaved image (column c of row r at (r >> 1) 2 d + (r & 1) 32 + c + (c >> 5) 32) -> [rows, d]"""
    return buf.reshape(rows // 2, d // 32, 2, 32).permute(0, 2, 1, 3).reshape(rows, d)


def v_image(src, col0, B, N, Npad, kvh, hd):
    """the V^T image [B, kvh, hd, Npad] (keys permuted inside every 16, padding zero): the permutation of test_v_transpose_is_exact"""
    v = src.cpu()[:, col0:col0 + kvh * hd].view(B, N, kvh, hd).permute(0, 2, 3, 1)
    want = torch.zeros(B, kvh, hd, Npad, dtype=torch.bfloat16)
    idx = torch.arange(Npad)
    pos = (idx & ~12) | ((idx & 4) << 1) | ((idx & 8) >> 1)
    valid = idx < N
    want[..., pos[valid]] = v[..., idx[valid]]
    return want


def ref_qstat(partials, width, eps):
    """(mean, rstd, mean_bound, rstd_bound) float64 [rows] from [rows, slots, 2] (sum, sum of squares) partials: var = E[x^2] - mean^2"""
    p = d64(partials)
    mean, e2 = p[..., 0].sum(-1) / width, p[..., 1].sum(-1) / width
    var = (e2 - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + f32(eps))
    mb = QSTAT_SUM * p[..., 0].abs().sum(-1) / width
    mabs = p[..., 0].abs().sum(-1) / width
    rb = rstd * (0.5 * (QSTAT_SUM * e2 + 2 * QSTAT_SUM * mabs * mabs + MARGIN * 2 * U * (e2 + mean * mean)) / (var + f32(eps)) + MARGIN * 2 * U)
    return mean, rstd, mb, rb


# ---- routing on the way out --------------------------------------------------------------------------------------------------------------
def _top2(logit):
    """moe_route.h: top-2, lowest index wins ties"""
    E = len(logit)
    i1 = 0
    for e in range(1, E):
        if logit[e] > logit[i1]:
            i1 = e
    i2 = 1 if i1 == 0 else 0
    for e in range(E):
        if e != i1 and e != i2 and logit[e] > logit[i2]:
            i2 = e
    return i1, i2


def check_routing(h_got, route_w, sel, wts, forced=None, what=""):
    """sel int [rows, 2], wts bf16 [rows, 2] against float64 logits of the h words the kernel wrote: logits = bf16(h . w_e) (ambiguous within
    the fp32 dot's bound: both neighbours tried), top-2 (either order where candidates tie), softmax over the two in float64 -> weights
    word for word (both neighbours within DELTA_ROUTE_W).  Returns the number of rows with an ambiguous logit."""
    import itertools
    h, w = d64(h_got), d64(route_w)
    E, d = w.shape
    exact = h @ w.t()
    bound = route_logit_delta(d) * (h.abs() @ w.abs().t())
    r, lo, hi, amb = neighbours(exact, bound / exact.abs().clamp_min(1e-300))
    sel, wts = sel.cpu().tolist(), wts.cpu().float().tolist()
    bad, namb = [], 0
    for row in range(h.shape[0]):
        opts = [([float(lo[row, e]), float(hi[row, e])] if bool(amb[row, e]) else [float(r[row, e])]) for e in range(E)]
        namb += int(bool(amb[row].any()))
        okay = False
        for logit in itertools.product(*opts):
            i1, i2 = (int(forced[row][0]), int(forced[row][1])) if forced is not None else _top2(logit)
            ex = math.exp(logit[i2] - logit[i1])
            wa, wb = 1.0 / (1.0 + ex), ex / (1.0 + ex)
            if i2 < i1:
                i1, i2, wa, wb = i2, i1, wb, wa
            if sel[row] != [i1, i2]:
                continue
            good = True
            for got, val in ((wts[row][0], wa), (wts[row][1], wb)):
                q = neighbours(torch.tensor([val], dtype=torch.float64), DELTA_ROUTE_W)
                good &= got == float(q[0]) or (bool(q[3]) and got in (float(q[1]), float(q[2])))
            okay |= good
        if not okay:
            bad.append((row, sel[row], wts[row], [float(v) for v in exact[row]]))
    if bad:
        raise AssertionError(f"{what}: routing wrong on {len(bad)} of {h.shape[0]} rows; first (row, sel, wts, float64 logits): {bad[:3]}")
    return namb


# ---- comparator --------------------------------------------------------------------------------------------------------------------------
def _top(name, keys, k=6):
    vals, counts = torch.unique(keys, return_counts=True)
    order = torch.argsort(counts, descending=True)[:k]
    return f"{name} {{" + ", ".join(f"{int(vals[i])}: {int(counts[i])}" for i in order.tolist()) + ("}" if len(vals) <= k else f", ... {len(vals)} values}}")


def wrong_mask(got, ch):
    """bool [rows, d]: words of got that equal no candidate of the chain (NaN - an unwritten word - equals none)"""
    g = got.detach().cpu().double()
    if ch.cands is None:
        return ~((g >= ch.lo) & (g <= ch.hi))
    good = torch.zeros_like(ch.amb)
    for c in ch.cands:
        good |= g == c
    return ~good


def assert_row_words(got, ch, what="", N=None, hd=None):
    """every word of got (bf16 [rows, d], logical layout) must equal one candidate of the chain.  Returns the ambiguous share.  The failure
    message names the count, the NaN / unwritten count, the first four words (got / want / float64) and the wrong words by sample, row,
    row % 4 (wave of norm.hip), row % 8 (workgroup of qkv_post.hip), 8-column chunk with its lane (chunk % 64) and round (chunk / 64), and head."""
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == tuple(ch.amb.shape), (got.dtype, got.shape, ch.amb.shape)
    share = float(ch.amb.double().mean())
    if share > MAX_AMBIGUOUS:
        raise PreconditionError(f"{what}: {share:.2%} of the words lie within the stage bounds of a bf16 midpoint (cap {MAX_AMBIGUOUS:.0%})")
    g = got.double()
    bad = wrong_mask(got, ch)
    n = int(bad.sum())
    if n == 0:
        return share
    idx = bad.nonzero()
    rows, cols = idx[:, 0], idx[:, 1]
    want = ch.want
    first = [f"(row {r}, col {c}: got {float(g[r, c])}, want {float(want[r, c])}, float64 {float(ch.first[r, c]):.9g})" for r, c in idx[:4].tolist()]
    chunk = cols // 8
    groups = [_top("row", rows), f"row % 4 {_runs(torch.bincount(rows % 4, minlength=4))}", f"row % 8 {_runs(torch.bincount(rows % 8, minlength=8))}",
              _top("chunk", chunk), _top("lane", chunk % 64), _top("chunk / 64", chunk // 64), _top("col % 64 / 32 (pair piece)", (cols % 64) // 32)]
    if N:
        groups.insert(0, _top("sample", rows // N))
    if hd:
        groups.append(_top("head", cols // hd))
    nan = int(torch.isnan(g)[bad].sum())
    raise AssertionError(f"{what}: {n} of {bad.numel()} words wrong ({nan} unwritten / NaN, {int((bad & ch.amb).sum())} of them ambiguous words outside "
                         f"every candidate; ambiguous share {share:.3%}); first: " + "; ".join(first) + "; by " + "; ".join(groups))


class GuardedBuf:
    """an output of n bf16 words, NaN-filled, between two guard zones of GUARD (7.0) that must survive the launch"""

    def __init__(self, n, device="cuda", zone=4096, dtype=torch.bfloat16, fill=float("nan")):
        self.zone, self.n = zone, n
        self.buf = torch.full((n + 2 * zone,), GUARD, device=device, dtype=dtype)
        self.out = self.buf[zone:zone + n]
        self.out.fill_(fill)

    def assert_intact(self, what=""):
        lo, hi = self.buf[:self.zone], self.buf[self.zone + self.n:]
        nlo, nhi = int((lo != GUARD).sum()), int((hi != GUARD).sum())
        if nlo or nhi:
            where = int((hi != GUARD).nonzero()[0]) if nhi else int((lo != GUARD).nonzero()[0]) - self.zone
            raise AssertionError(f"{what}: stray stores outside the buffer: {nlo} words before it, {nhi} behind it (first at {where:+d} words)")


def guarded_copy(t, device="cuda"):
    """an input / in-place tensor between guard zones: (GuardedBuf, view shaped like t)"""
    g = GuardedBuf(t.numel(), device=device, dtype=t.dtype, fill=0.0)
    g.out.copy_(t.reshape(-1))
    return g, g.out.view(t.shape)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def draw_rows(rows, d, seed, std=3.0, mean_rows=False, device="cpu"):
    """bf16 [rows, d] N(0, std^2); every fifth row carries one large outlier (40 std); mean_rows: every third row a mean of one std"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g) * std
    for r in range(0, rows, 5):
        x[r, (7 * r + 3) % d] = 40.0 * std
    if mean_rows:
        x[1::3] += std
    return x.to(torch.bfloat16).to(device)


def draw_vec(n, seed, centre=0.0, std=0.1, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (centre + std * torch.randn(n, generator=g)).to(torch.bfloat16).to(device)


def draw_mod(B, ld, seed, std=0.3, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, ld, generator=g) * std).to(torch.bfloat16).to(device)


# ---- fp32 emulations (CPU tests: the chains as an fp32 machine runs them, with planted faults) ----------------------------------------------
def _r16(t):
    return t.to(torch.bfloat16).float()


def _butterfly(v):
    """wave_sum of common.h over the last axis (64 lanes): xor 1, xor 2, half mirror, mirror, then (r0 + r16) + (r32 + r48)"""
    v = v.reshape(*v.shape[:-1], 4, 2, 2, 2, 2)
    v = v[..., 0] + v[..., 1]
    v = v[..., 0] + v[..., 1]
    v = v[..., 0] + v[..., 1]
    v = v[..., 0] + v[..., 1]
    return (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])


def _lanes(x):
    """[rows, d] fp32 -> [rows, chunk round i, lane, 8] zero-padded (load_row)"""
    rows, d = x.shape
    m = maxch(d)
    pad = torch.zeros(rows, m * 512, dtype=x.dtype)
    pad[:, :d] = x
    return pad.view(rows, m, 64, 8)


def emu_sumsq(x, order="kernel", drop=None):
    """fp32 sum of squares of bf16 rows [rows, d] -> [rows, 1].  kernel: row_sumsq (four v_dot2 accumulators per lane, two roundings per
    step, tree, butterfly); serial: left to right; pairwise: torch.sum.  drop = (row, col): that element is missing from the sum"""
    x = x.float().clone()
    if drop is not None:
        x[drop[0], drop[1]] = 0.0
    if order == "serial":
        return torch.cumsum(x * x, -1)[:, -1:]      # (torch's fp32 cumsum adds left to right)
    if order == "pairwise":
        return (x * x).sum(-1, keepdim=True)
    v = _lanes(x)
    s = torch.zeros(x.shape[0], 64, 4)
    for i in range(v.shape[1]):
        lo, hi = v[:, i, :, 0::2], v[:, i, :, 1::2]
        s = (s + lo * lo) + hi * hi
    return _butterfly((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])).unsqueeze(-1)


def emu_sum(x, order="kernel"):
    x = x.float()
    if order == "serial":
        return torch.cumsum(x, -1)[:, -1:]
    if order == "pairwise":
        return x.sum(-1, keepdim=True)
    v = _lanes(x)
    s = torch.zeros(x.shape[0], 64, 2)
    for i in range(v.shape[1]):
        for k in range(4):
            s = s + v[:, i, :, 2 * k:2 * k + 2]
    return _butterfly(s[..., 0] + s[..., 1]).unsqueeze(-1)


def emu_rinv(x, eps, order="kernel", drop=None):
    return torch.rsqrt(emu_sumsq(x, order, drop) / float(x.shape[1]) + torch.tensor(eps, dtype=torch.float32))


def emu_rms_mod(x, rinv, w, scale, shift, scale_pre=0, apex=0, fault=None):
    """apply_rms_mod_store in fp32; scale / shift per row.  fault 'no_round_one_plus': (1 + scale) kept in fp32"""
    n = x.float() * rinv
    if w is not None:
        n = (n if apex else _r16(n)) * w.float()
    if scale is not None:
        s1 = scale.float() if scale_pre else (1.0 + scale.float() if fault == "no_round_one_plus" else _r16(1.0 + scale.float()))
        n = _r16(n) * s1
    if shift is not None:
        n = _r16(n) + shift.float()
    return n.to(torch.bfloat16)


def emu_rmsnorm_mod(x, w, scale, shift, B, N, eps, scale_pre=0, apex=0, order="kernel", fault=None, drop=None):
    sc, sh = _per_row(scale, B, N), _per_row(shift, B, N)
    if fault == "boundary_scale" and sc is not None:      # the last row of sample 0 is modulated with sample 1's vector
        sc = sc.clone()
        sc[N - 1] = scale[1]
    return emu_rms_mod(x, emu_rinv(x, eps, order, drop), w, sc, sh, scale_pre, apex, fault)


def emu_moe_combine(ys, pos, wts, fault=None):
    pos = pos.long()
    wts = wts.float()
    if fault == "moe_wrong_row":                          # row 2 pairs its weights with the expert rows the other way round
        pos = pos.clone()
        pos[2] = pos[2].flip(0)
    a, b = _r16(wts[:, 0:1] * ys.float()[pos[:, 0]]), _r16(wts[:, 1:2] * ys.float()[pos[:, 1]])
    return _r16(_r16(0.0 + a) + b).to(torch.bfloat16)


def emu_gated(x, y, post_w, gate, next_w, next_scale, next_shift, B, N, eps, eps_next, post_mode, next_mode, scale_pre=1, apex=0, order="kernel",
              ystat=None):
    """gated_residual_norm_kernel in fp32 (gate prepared or None) -> (x', h or None)"""
    yn = y.float()
    if post_mode == 1:
        if ystat is not None:
            ss = torch.zeros(y.shape[0], 1)
            for s in range(0, ystat.shape[1], 2):
                ss = ss + (ystat[:, s:s + 1] + ystat[:, s + 1:s + 2])
            rinv = torch.rsqrt(ss / float(y.shape[1]) + torch.tensor(eps, dtype=torch.float32))
        else:
            rinv = emu_rinv(y, eps, order)
        yn = _r16((yn * rinv if apex else _r16(yn * rinv)) * post_w.float())
    if gate is not None:
        yn = _r16(_per_row(gate, B, N).float() * yn)
    xn = (x.float() + yn).to(torch.bfloat16)
    if next_mode == 0:
        return xn, None
    sc, sh = _per_row(next_scale, B, N), _per_row(next_shift, B, N)
    if next_mode == 1:
        return xn, emu_rms_mod(xn, emu_rinv(xn, eps, order), next_w, sc, sh, scale_pre, apex)
    xf = xn.float()
    mean = emu_sum(xf, order) / float(xf.shape[1])
    dl = xf - mean
    rstd = torch.rsqrt(emu_sum(dl * dl, order) / float(xf.shape[1]) + torch.tensor(eps_next, dtype=torch.float32))
    n = dl * rstd
    if sc is not None:
        n = n * (sc.float() if scale_pre else _r16(1.0 + sc.float()))
    if sh is not None:
        n = n + sh.float()
    return xn, n.to(torch.bfloat16)


def emu_qk_norm_rope(src, col0, ln_w, ln_b, ln_eps, B, N, heads, hd, rope_mode, table, branch, grid_w, out_scale=1.0, n_tok_b=None, grid_w_b=None,
                     order="kernel", fault=None):
    """qk_norm_rope in fp32 -> bf16 logical [B * N, heads * hd]"""
    width = heads * hd
    y = src.float()[:, col0:col0 + width]
    if ln_w is not None:
        mean = emu_sum(y, order) / float(width)
        dl = y - mean
        rstd = torch.rsqrt(emu_sum(dl * dl, order) / float(width) + torch.tensor(ln_eps, dtype=torch.float32))
        y = dl * rstd * ln_w.float() + ln_b.float()
    if rope_mode != 0:
        cos, sin = rope_factors(table, branch, B, N, hd, rope_mode, grid_w, n_tok_b, grid_w_b, fault)
        cos, sin = cos.float()[:, None, :], sin.float()[:, None, :]
        y4 = y.reshape(B * N, heads, hd // 2, 2)
        y = torch.stack([y4[..., 0] * cos - y4[..., 1] * sin, y4[..., 0] * sin + y4[..., 1] * cos], -1).reshape(B * N, width)
    if f32(out_scale) != 1.0:
        y = y * torch.tensor(out_scale, dtype=torch.float32)
    return y.to(torch.bfloat16)
