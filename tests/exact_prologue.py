"""Exact checks of the attention launches that build q (and k, V^T) themselves: generators of the RAW operands, fp32 restatements of the two
prologues and the launches (plain module, no test in here).

AttnArgs::q_raw of attn_fwd_kernel_v4<72> and attn_small_fused_kernel<48> do LayerNorm + 2-D RoPE (+ the K scale) in front of the attention
loop.  Both can be fed so that they must produce, bit for bit, the integer q / k of tests/exact_attention.py:
  * the RoPE table is an input: entries that are quarter turns (1, 0), (0, 1), (-1, 0), (0, -1), chosen per (branch, position, frequency) by
    an integer hash, make the rotation a signed swap - exact in fp32 with or without contraction;
  * LayerNorm weights are powers of two, biases small integers, and the statistics are chosen, not computed: the raw value of a word is
    x = (target - b) / (rstd w) + mean, rounded to bf16; ((x - mean) rstd) w + b is then exact in fp32 (every factor a power of two, every
    sum of a few bits) and the ONE bf16 rounding behind the rotation must give the integer target.  `determined()` checks that word by word
    in float64, for every word of every case (cap 0): a case whose raw buffer does not pin every word is a PreconditionError.
    - q_raw path: (mean, rstd) are read as given: mean in {-3 .. 3}, rstd in {2^-3 .. 2^-6} per row by hash.  Where a word cannot be pinned
      (x needs more than bf16's 8 bits and the rounding moves the result across a midpoint) the channel's bias falls back to its sign, then
      to 0, and the row's mean to 0; every case asserts that two thirds of the rows keep a non-zero mean and 18 of 72 channels per head a bias.
    - small kernel: the statistics arrive as per-tile (sum, sum of squares) partials.  The sums add to exactly 0, the squares to exactly
      W 4^5 (W the projection width), integers spread unevenly over the slots; rstd is then 2^-5 (1 + e) with |e| <= 2^-20 (fl(1 / W), one
      product, eps = 1e-5 below half an ulp of 1024, a 1-ulp rsqrt; margin 4) and `determined()` evaluates the chain at both ends of
      that interval.  A zero target under a non-zero bias would come out as -b e, so the bias is non-zero exactly on the channels where no
      token's target is zero.
  * exact_attention's generators permute the reduction dims per sample; `align_samples` applies one more joint permutation of q's and k's
    dims (scores unchanged) so that every sample of a (kv-)head uses sample 0's placement - LayerNorm vectors are per channel, not per sample.
The expected output is exact_attention.expected() on the generator's own q, k, v and the comparator is assert_attention_words, unchanged."""
import torch

import exact_attention as X
from exact_operands import Guarded, PreconditionError

J = 5                         # small kernel: rstd = 2^-J
EPS_RSTD = 2.0 ** -20
POISON_STAT = 1.0e30
WEIGHTS = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5)
# q_raw coverage floors after the relaxations of qraw_from_target.  6 of 7 hashed means are non-zero (86 %), 8 of 9 hashed biases; the cases
# keep 69 .. 91 % of the rows and 20 .. 51 of 72 channels per head (the selector's digit dims hold zeros, which pin a bias to |b| <= 1).
# Floors: two thirds of the rows, a quarter of a head's channels - a generator change that loses the coverage fails every case
QRAW_MIN_ROWS_WITH_MEAN = 2 / 3
QRAW_MIN_BIASED_CHANNELS = 18

# the cases of tests/test_gpu_prologue_exact.py (and, one for one, of tests/test_exact_prologue_cpu.py)
QRAW_SHAPES = [(1, 4, 4, 64, 8), (2, 4, 1, 192, 16), (1, 8, 2, 320, 20), (1, 2, 2, 1024, 32), (1, 2, 1, 4160, 65)]   # B, H, Hkv, N, grid_w
QRAW_T = ["below", "above", "null"]
# with fused text: B = 2, both valid lengths, on the first three shapes (MHA, MQA, GQA); one (T, valid) per shape also above the watershed
QRAW_TEXT = [((2,) + shape[1:], T, valid, tname) for i, shape in enumerate(QRAW_SHAPES[:3])
             for j, (T, valid) in enumerate([(77, (77, 1)), (128, (128, 8)), (200, (60, 130))]) for tname in (("below", "above") if i == j else ("below",))]
SMALL_SHAPES = [(1, 64, 8, 8, 8), (2, 128, 8, 8, 16), (3, 192, 16, 8, 12), (1, 512, 16, 8, 32), (2, 256, 32, 32, 16)]   # B, tokens, H, Hkv, grid_w
K_SCALES = [0.5, 1.0, 2.0]
WATERSHED = 0.5
T_VALUE = {"below": 0.25, "above": 0.75, "null": None}


def case_seed(*shape):
    return sum(shape) + len(shape)


def branch_of(t):
    return 1 if t is None or not t < WATERSHED else 0


def table_len(N, grid_w):
    """longer than both sides of the token grid"""
    return max(grid_w, (N + grid_w - 1) // grid_w) + 3


# ---- the table --------------------------------------------------------------------------------------------------------------------------
def quarter_turn_table(branches, length, hd, seed, device="cpu"):
    """([branches][length][hd / 4][2], its transpose [branches][hd / 4][length][2]) float32 (cos, sin): quarter turns by hash; two branches
    differ at every (position, frequency)"""
    nf = hd // 4
    p, f = X._ar(length, device)[:, None], X._ar(nf, device)[None, :]
    qt0 = X._mix(p * 64 + f, seed) % 4
    step = 1 + X._mix(p * 64 + f, seed + 1) % 3
    qt = torch.stack([(qt0 + b * step) % 4 for b in range(branches)])
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0], device=device)[qt]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0], device=device)[qt]
    table = torch.stack([cos, sin], -1).float().contiguous()
    return table, table.permute(0, 2, 1, 3).contiguous()


def _factors(table, branch, N, grid_w, hd, fault=None):
    """(cos, sin) [N, hd / 2] of the documented convention: complex slot pr = d / 2 turns at frequency pr >> 1 with the row position n / grid_w
    (pr even) or the column position n % grid_w (pr odd).  fault: a planted error of tests/test_exact_prologue_cpu.py"""
    dev = table.device
    n, pr = X._ar(N, dev)[:, None], X._ar(hd // 2, dev)[None, :]
    f = (pr >> 1).expand(N, -1).clone()
    gw = grid_w + 1 if fault == "grid_w" else grid_w
    row, col = n // gw, n % gw
    if fault == "rowcol":
        row, col = col, row
    if fault == "freq":
        f[:, 2] = f[:, 2] + 1
    pos = torch.where(pr % 2 == 0, row, col)
    br = 1 - branch if fault == "branch" else branch
    cs = table[br, pos, f]
    return cs[..., 0], cs[..., 1]


def rotate(y, table, branch, grid_w, fma=False, fault=None):
    """the kernels' rotation in fp32 on y [..., N, hd]: (y0 c - y1 s, y0 s + y1 c), plain or with the second product contracted into an fma"""
    N, hd = y.shape[-2], y.shape[-1]
    c, s = _factors(table, branch, N, grid_w, hd, fault)
    y0, y1 = y[..., 0::2], y[..., 1::2]
    if fma:
        o0 = (y0.double() * c.double() - (y1 * s).double()).float()
        o1 = (y0.double() * s.double() + (y1 * c).double()).float()
    else:
        o0, o1 = y0 * c - y1 * s, y0 * s + y1 * c
    return torch.stack([o0, o1], -1).flatten(-2)


def unrotate(target, table, branch, grid_w):
    """the inverse signed swap by plain indexing: [..., N, hd] -> what must enter the rotation for `target` to leave it"""
    N, hd = target.shape[-2], target.shape[-1]
    c, s = _factors(table, branch, N, grid_w, hd)
    qt = torch.where(c == 1, 0, torch.where(s == 1, 1, torch.where(c == -1, 2, 3)))
    o0, o1 = target[..., 0::2], target[..., 1::2]
    y0 = torch.where(qt == 0, o0, torch.where(qt == 1, o1, torch.where(qt == 2, -o0, -o1)))
    y1 = torch.where(qt == 0, o1, torch.where(qt == 1, -o0, torch.where(qt == 2, -o1, o0)))
    return torch.stack([y0, y1], -1).flatten(-2)


# ---- generator side ---------------------------------------------------------------------------------------------------------------------
def align_samples(inp, seed, txt=None):
    """samples b >= 1 take sample 0's placement of the logical reduction dims (a joint permutation of q's and k's last axis per kv-head);
    txt: the text operands of a fused draw (same q, their own k), permuted along"""
    sides = [inp] + ([txt] if txt is not None else [])
    q, ks = inp["q"].clone(), [s["k"].clone() for s in sides]
    B, H, _, hd = q.shape
    Hkv = ks[0].shape[1]
    rep = H // Hkv
    for b in range(1, B):
        for kvh in range(Hkv):
            pb, p0 = X._dim_perm(hd, b, kvh, seed, q.device), X._dim_perm(hd, 0, kvh, seed, q.device)
            for k, s in zip(ks, sides):
                k[b, kvh][:, p0] = s["k"][b, kvh][:, pb]
            for h in range(kvh * rep, (kvh + 1) * rep):
                q[b, h][:, p0] = inp["q"][b, h][:, pb]
    # ... and the dims of a kv-head are placed so that the channels without a zero (in q, in k) fill whole complex slots - the rotation mixes
    # the two channels of a slot, and only a slot free of zeros can carry a bias on the small kernel; the slots are then shuffled by hash
    q2, ks2 = q.clone(), [k.clone() for k in ks]
    for kvh in range(Hkv):
        hs = slice(kvh * rep, (kvh + 1) * rep)
        zq = (q[:, hs] != 0).flatten(0, 2).all(0)
        zk = torch.stack([(k[:, kvh] != 0).flatten(0, 1).all(0) for k in ks]).all(0)
        order = torch.argsort(-(2 * zq.long() + zk.long()), stable=True)
        slots = torch.argsort(X._mix(X._ar(hd // 2, q.device) + 64 * kvh, seed + 13))
        idx = order.view(hd // 2, 2)[slots].flatten()
        q2[:, hs] = q[:, hs][..., idx]
        for k2, k in zip(ks2, ks):
            k2[:, kvh] = k[:, kvh][..., idx]
    for s, k2 in zip(sides, ks2):
        s["q"], s["k"] = q2, k2
    return inp


def draw(family, B, H, Hkv, N, hd, seed, device="cpu"):
    return align_samples(X.GENERATORS[family](B, H, Hkv, N, N, hd, seed=seed, device=device), seed)


def draw_fused(family, B, H, Hkv, N, T, hd, seed, valid, device="cpu"):
    a, t = X.fused_draw(family, B, H, Hkv, N, T, hd, seed, valid, device)
    align_samples(a, seed, t)
    return a, t


def _hash_pick(values, idx, seed, device):
    return torch.tensor(values, dtype=torch.float64, device=device)[X._mix(idx, seed) % len(values)]


def _r16(x):
    return x.to(torch.bfloat16).double()


def _bf16_step(x, up):
    """the bf16 neighbour above / below a bf16-valued float64 tensor"""
    i = x.to(torch.bfloat16).view(torch.int16).to(torch.int32)
    away = (x > 0) == up
    j = torch.where(x == 0, i, torch.where(away, i + 1, i - 1))   # (sign-magnitude words; a zero stays: its raw value is exact anyway)
    return j.to(torch.int16).view(torch.bfloat16).double()


def chain64(x, mean, rstd, w, b, k_scale=1.0):
    """((x - mean) rstd) w + b, times k_scale, in float64 (what the fp32 chain computes exactly on these operands), before the one rounding"""
    return (((x - mean) * rstd) * w + b) * k_scale


def determined(x, mean, rstd, w, b, target, k_scale=1.0, eps=0.0):
    """bool per word: the chain at rstd (1 - eps) and rstd (1 + eps) rounds to the same bf16 word, that word is the integer target, and an
    exact zero is exactly zero.  (The rotation behind the chain is a signed swap: it commutes with the rounding.)"""
    lo, hi = chain64(x, mean, rstd * (1 - eps), w, b, k_scale), chain64(x, mean, rstd * (1 + eps), w, b, k_scale)
    good = (_r16(lo) == target) & (_r16(hi) == target)
    return good & ((target != 0) | ((lo == 0) & (hi == 0)))


def _solve(yt, mean, rstd, w, b):
    """(x bf16-valued float64, solved bool): RN_bf16 of the ideal raw value or, where that one lands across a midpoint, a bf16 neighbour"""
    ideal = (yt - b) / (rstd * w) + mean
    x0 = _r16(ideal)
    x, ok = x0.clone(), determined(x0, mean, rstd, w, b, yt)
    for cand in (_bf16_step(x0, True), _bf16_step(x0, False)):
        take = ~ok & determined(cand, mean, rstd, w, b, yt)
        x = torch.where(take, cand, x)
        ok |= take
    return x, ok


def qraw_from_target(q, table, branch, grid_w, seed):
    """the raw operands of the q_raw prologue for integer targets q [B, H, N, hd]: dict(qkv [B * N, ld] bf16 (NaN in every column no operand
    owns), ld, q_col0, stat [B * N, 2] fp32 (mean, rstd), w, b [H * hd] bf16, and x, mean, rstd, yt (float64 views for determined()))"""
    B, H, N, hd = q.shape
    dev = q.device
    yt = unrotate(q.double(), table.double(), branch, grid_w)
    ch = X._ar(H * hd, dev)
    w = _hash_pick(WEIGHTS, ch, seed + 21, dev).view(1, H, 1, hd)
    b = (X._mix(ch, seed + 22) % 9 - 4).double().view(1, H, 1, hd)
    rows = X._ar(B * N, dev)
    mean = (X._mix(rows, seed + 23) % 7 - 3).double().view(B, 1, N, 1)
    rstd = torch.exp2(-(3 + X._mix(rows, seed + 24) % 4).double()).view(B, 1, N, 1)
    # relaxations, in order, each applied only where a word is still not pinned: a channel's bias -> its sign -> 0, a row's mean -> 0 (x =
    # (target - b) 2^k is then exact), and once more the bias -> 0 for channels the changed rows have unsettled
    sign_b = torch.sign(b)
    x, ok = _solve(yt, mean, rstd, w, b)
    for what in ("bias_sign", "bias_zero", "mean_zero", "bias_zero"):
        if bool(ok.all()):
            break
        if what == "mean_zero":
            mean = torch.where((~ok).any(1, keepdim=True).any(3, keepdim=True), torch.zeros_like(mean), mean)
        else:
            bad_ch = (~ok).any(0, keepdim=True).any(2, keepdim=True)
            b = torch.where(bad_ch, sign_b if what == "bias_sign" else torch.zeros_like(b), b)
        x, ok = _solve(yt, mean, rstd, w, b)
    if not bool(ok.all()):
        raise PreconditionError(f"q_raw: {int((~ok).sum())} words are not determined (cap 0)")
    rows_mean, ch_bias = float((mean != 0).double().mean()), int((b != 0).sum(3).min())
    if rows_mean < QRAW_MIN_ROWS_WITH_MEAN:
        raise PreconditionError(f"q_raw: only {rows_mean:.1%} of the rows keep a non-zero mean (floor {QRAW_MIN_ROWS_WITH_MEAN:.0%})")
    if ch_bias < QRAW_MIN_BIASED_CHANNELS:
        raise PreconditionError(f"q_raw: a head with only {ch_bias} channels under a non-zero bias (floor {QRAW_MIN_BIASED_CHANNELS})")
    q_col0, ld = 16, 16 + H * hd + 24
    qkv = torch.full((B * N, ld), float("nan"), dtype=torch.bfloat16, device=dev)
    qkv[:, q_col0:q_col0 + H * hd] = x.permute(0, 2, 1, 3).reshape(B * N, H * hd).to(torch.bfloat16)
    stat = torch.stack([mean.expand(B, 1, N, 1).reshape(-1), rstd.reshape(-1)], -1).float().contiguous()
    return dict(qkv=qkv, ld=ld, q_col0=q_col0, stat=stat, w=w.reshape(-1).to(torch.bfloat16), b=b.reshape(-1).to(torch.bfloat16),
                x=x, mean=mean, rstd=rstd, wd=w, bd=b, yt=yt, table=table, branch=branch, grid_w=grid_w, rows_mean=rows_mean, ch_bias=ch_bias)


def _stat_slots(nslot, W, dev):
    """(sum, sum of squares) partials of one row over nslot slots: the sums add to 0, the squares to W 4^J; the first and the last slot hold
    W 2^6 / - W 2^6 and a quarter of the squares each (one slot too few moves the mean by 64 and the variance by a factor >= 1.25)"""
    s1, s2 = [0.0] * nslot, [0.0] * nslot
    T = W * 4 ** J
    s1[0], s1[-1] = W * 64.0, -W * 64.0
    s2[0], s2[-1] = T / 4, T / 4
    mid = nslot - 2
    rest = T / 2
    for i in range(mid):
        s1[1 + i] = W * 8.0 * (0 if (i == mid - 1 and mid % 2) else (1 if i % 2 == 0 else -1))
        share = rest if i == mid - 1 else rest / 2
        s2[1 + i] = share
        rest -= share
    assert nslot >= 3 and sum(s1) == 0 and sum(s2) == T and all(v == int(v) and v > 0 for v in s2)
    return torch.tensor([s1, s2], dtype=torch.float32, device=dev).t().contiguous()   # [nslot, 2]


def small_from_target(q, k, v, table, branch, grid_w, k_scale, seed):
    """the raw operands of attn_small_fused_kernel for integer targets q [B, H, N, hd], k, v [B, Hkv, N, hd] (see the module docstring)"""
    B, H, N, hd = q.shape
    Hkv = k.shape[1]
    dev = q.device
    d, dkv = H * hd, Hkv * hd
    out = dict(table=table, branch=branch, grid_w=grid_w, k_scale=k_scale)
    parts = {}
    for name, tgt, heads, ks, sd in (("q", q, H, 1.0, 31), ("k", k, Hkv, k_scale, 41)):
        yt = unrotate(tgt.double(), table.double(), branch, grid_w)
        ch = X._ar(heads * hd, dev)
        w = _hash_pick(WEIGHTS, ch, seed + sd, dev).view(1, heads, 1, hd)
        b = (1 + X._mix(ch, seed + sd + 1) % 4).double() * (1 - 2 * (X._mix(ch, seed + sd + 2) & 1).double())
        has_zero = (yt == 0).any(0, keepdim=True).any(2, keepdim=True)
        b = torch.where(has_zero, torch.zeros_like(w), b.view(1, heads, 1, hd))      # integer bias of the effective (scaled) value
        x = (yt - b) * 2.0 ** J / (w * ks)
        if not torch.equal(_r16(x), x):
            raise PreconditionError(f"small kernel: raw {name} values that do not fit bf16")
        zero, rstd = torch.zeros(1, dtype=torch.float64, device=dev), torch.full((1,), 2.0 ** -J, dtype=torch.float64, device=dev)
        ok = determined(x, zero, rstd, w, b / ks, yt, ks, EPS_RSTD)
        if not bool(ok.all()):
            raise PreconditionError(f"small kernel: {int((~ok).sum())} {name} words are not determined (cap 0)")
        parts[name] = dict(x=x, w=w, b=b / ks, yt=yt)
    nzq, nzk = int((parts["q"]["b"] != 0).sum(3).min()), float((parts["k"]["b"] != 0).double().mean())
    if nzq < 4 or nzk < 0.5:
        raise PreconditionError(f"small kernel: non-zero bias on {nzq} q channels of some head, {nzk:.1%} of the k channels")
    q_col0, k_col0 = 8, 8 + d + 8
    v_col0 = k_col0 + dkv + 8
    ld = v_col0 + dkv + 8
    qkv = torch.full((B * N, ld), float("nan"), dtype=torch.bfloat16, device=dev)
    qkv[:, q_col0:q_col0 + d] = parts["q"]["x"].permute(0, 2, 1, 3).reshape(B * N, d).to(torch.bfloat16)
    qkv[:, k_col0:k_col0 + dkv] = parts["k"]["x"].permute(0, 2, 1, 3).reshape(B * N, dkv).to(torch.bfloat16)
    qkv[:, v_col0:v_col0 + dkv] = v.permute(0, 2, 1, 3).reshape(B * N, dkv)
    q_nslot, k_nslot = d // 128, dkv // 128
    q_slot0, k_slot0 = 1, 1 + q_nslot + 1
    slots = k_slot0 + k_nslot + k_nslot + 1                                            # | poison | q | poison | k | v (poison) | poison |
    rowstat = torch.full((B * N, slots, 2), POISON_STAT, dtype=torch.float32, device=dev)
    rowstat[:, q_slot0:q_slot0 + q_nslot] = _stat_slots(q_nslot, d, dev)
    rowstat[:, k_slot0:k_slot0 + k_nslot] = _stat_slots(k_nslot, dkv, dev)
    bf = lambda t: t.reshape(-1).to(torch.bfloat16)
    out.update(qkv=qkv, ld=ld, q_col0=q_col0, k_col0=k_col0, v_col0=v_col0, rowstat=rowstat, slots=slots, q_slot0=q_slot0, q_nslot=q_nslot,
               k_slot0=k_slot0, k_nslot=k_nslot, qw=bf(parts["q"]["w"]), qb=bf(parts["q"]["b"]), kw=bf(parts["k"]["w"]), kb=bf(parts["k"]["b"]),
               shape=(B, H, Hkv, N, hd))
    if not (torch.equal(out["qb"].double(), parts["q"]["b"].reshape(-1)) and torch.equal(out["kb"].double(), parts["k"]["b"].reshape(-1))):
        raise PreconditionError("small kernel: a bias that does not fit bf16")
    return out


# ---- fp32 restatements of the prologues (torch, any device) and the planted faults ------------------------------------------------------
def _ln32(x, mean, rstd, w, b, fma):
    t = (x - mean) * rstd
    return (t.double() * w.double() + b.double()).float() if fma else t * w + b


def _heads_view(vec, heads, hd, fault_head=None):
    """[heads * hd] -> [1, heads, 1, hd]; fault_head: that head reads the vector of head + 1"""
    m = vec.float().view(heads, hd).clone()
    if fault_head is not None:
        m[fault_head] = vec.float().view(heads, hd)[(fault_head + 1) % heads]
    return m.view(1, heads, 1, hd)


def _merge_head(clean, faulty, head):
    out = clean.clone()
    out[:, head] = faulty[:, head]
    return out


def restate_qraw(raw, B, H, hd, t=None, fma=False, fault=None, fault_head=0):
    """q [B, H, N, hd] bf16 as the q_raw prologue states it (attention_v4.hip: ((x - mean) rstd) w + b, rotation, one rounding), from the raw
    buffers alone.  fault in {None, freq, rowcol, branch, grid_w, bias, weight}: planted on head fault_head"""
    qkv, stat = raw["qkv"], raw["stat"]
    BN = qkv.shape[0]
    x = qkv[:, raw["q_col0"]:raw["q_col0"] + H * hd].float()
    N = BN // B
    x = x.view(B, N, H, hd).permute(0, 2, 1, 3)
    mean, rstd = stat[:, 0].view(B, 1, N, 1), stat[:, 1].view(B, 1, N, 1)

    def run(f):
        w = _heads_view(raw["w"], H, hd, fault_head if f == "weight" else None)
        b = _heads_view(raw["b"], H, hd, fault_head if f == "bias" else None)
        y = _ln32(x, mean, rstd, w, b, fma)
        return rotate(y, raw["table"], branch_of(t), raw["grid_w"], fma, f).to(torch.bfloat16)
    clean = run(None)
    return clean if fault is None else _merge_head(clean, run(fault), fault_head)


def _row_stat32(part, nslot_lo, nslot_hi, W):
    """row_stat of attention_small.hip in fp32: (mean, rstd) from the slots [lo, hi)"""
    s = part[:, nslot_lo:nslot_hi].float().sum(1)
    inv_w = torch.tensor(1.0 / W, dtype=torch.float32, device=part.device)
    mean = s[:, 0] * inv_w
    var = torch.clamp(s[:, 1] * inv_w - mean * mean, min=0.0) + torch.tensor(1e-5, dtype=torch.float32, device=part.device)
    return mean, torch.rsqrt(var)


def restate_small(raw, t=None, fma=False, fault=None, fault_head=0):
    """(q [B, H, N, hd], k, v [B, Hkv, N, hd]) bf16 as attn_small_fused_kernel states them, from the raw buffers alone.  v is what the PV
    product multiplies key n's weight with (the key-permuted, swizzled LDS image read back).  fault in {None, freq, rowcol, branch, grid_w,
    bias, weight (on q), kfreq, krowcol, kbranch, kgrid_w, kbias (on k), stat_drop, stat_v, k_scale, v_keyperm, v_swizzle}: planted on (kv-)head fault_head"""
    B, H, Hkv, N, hd = raw["shape"]
    qkv, rs = raw["qkv"], raw["rowstat"]
    d, dkv = H * hd, Hkv * hd
    col = lambda c0, heads: qkv[:, c0:c0 + heads * hd].float().view(B, N, heads, hd).permute(0, 2, 1, 3)
    br = branch_of(t)

    def run(f):
        qm, qr = _row_stat32(rs, raw["q_slot0"], raw["q_slot0"] + raw["q_nslot"], d)
        k_hi = raw["k_slot0"] + raw["k_nslot"] + (-1 if f == "stat_drop" else 1 if f == "stat_v" else 0)
        km, kr = _row_stat32(rs, raw["k_slot0"], k_hi, dkv)
        qf = f if f in ("freq", "rowcol", "branch", "grid_w") else None
        kf = {"kfreq": "freq", "krowcol": "rowcol", "kbranch": "branch", "kgrid_w": "grid_w"}.get(f)
        yq = _ln32(col(raw["q_col0"], H), qm.view(B, 1, N, 1), qr.view(B, 1, N, 1), _heads_view(raw["qw"], H, hd, fault_head if f == "weight" else None),
                   _heads_view(raw["qb"], H, hd, fault_head if f == "bias" else None), fma)
        yk = _ln32(col(raw["k_col0"], Hkv), km.view(B, 1, N, 1), kr.view(B, 1, N, 1), _heads_view(raw["kw"], Hkv, hd),
                   _heads_view(raw["kb"], Hkv, hd, fault_head if f == "kbias" else None), fma)
        q = rotate(yq, raw["table"], br, raw["grid_w"], fma, qf).to(torch.bfloat16)
        ks = 1.0 if f == "k_scale" else raw["k_scale"]
        k = (rotate(yk, raw["table"], br, raw["grid_w"], fma, kf) * ks).to(torch.bfloat16)
        v = col(raw["v_col0"], Hkv).to(torch.bfloat16)
        n = X._ar(N, qkv.device)
        if f == "v_keyperm":      # the image written at position n instead of v_position(n): key n's weight meets the V row of v_position(n)
            v = v[:, :, X.v_position(n)]
        if f == "v_swizzle":      # row d = 2 written without the (d >> 1) & 7 chunk swizzle: the reader's slot holds the chunk 8 positions over
            dd = 2
            src_pos = X.v_position(n) ^ (((dd >> 1) & 7) << 3)
            src = X.v_position(src_pos)                      # v_position is its own inverse
            v = v.clone()
            v[:, :, :, dd] = v[:, :, src, dd]
        return q, k, v
    clean = run(None)
    if fault is None:
        return clean
    bad = run(fault)
    return tuple(_merge_head(c, b, fault_head) for c, b in zip(clean, bad))


def attention64(q, k, v, valid=None):
    """plain float64 base-2 softmax attention of bf16 q [B, H, N, hd], k, v [B, Hkv, Nk, hd] (scores q . k) -> float64 [B, H, N, hd]"""
    B, H, N, hd = q.shape
    rep = H // k.shape[1]
    kd, vd = k.double().repeat_interleave(rep, 1), v.double().repeat_interleave(rep, 1)
    s = q.double() @ kd.transpose(2, 3)
    if valid is not None:
        for b, nv in enumerate(valid):
            s[b, :, :, nv:] = float("-inf")
    w = torch.exp2(s - s.max(-1, keepdim=True).values)
    return (w @ vd) / w.sum(-1, keepdim=True)


# ---- launches (GPU) -----------------------------------------------------------------------------------------------------------------------
def _snapshot(tensors):
    return [None if t is None else t.clone() for t in tensors]


def _assert_unchanged(tensors, before, what):
    for i, (t, b) in enumerate(zip(tensors, before)):
        if t is not None:
            same = torch.equal(t.view(torch.int16), b.view(torch.int16)) if t.dtype == torch.bfloat16 else torch.equal(t.view(torch.int32), b.view(torch.int32))
            assert same, f"{what}: input {i} was written"


def run_qraw(raw, inp, t, txt=None, gate=None, what="", expect_refusal=False, grid_w=None, tlen=None):
    """lt_op_attention_qraw_ex on a guarded NaN-filled output -> bf16 [B, H, N, hd]; k, V^T (and the text operands) are finished operands"""
    from gpu_util import P, lib, ok, stream
    k = inp["k"].contiguous()
    B, Hkv, N, hd = k.shape
    H = inp["q"].shape[1]
    Nkpad = X.pad64(N)
    vt = X.make_vt(inp["v"], Nkpad)
    table, table_t = raw["table"], raw["table"].permute(0, 2, 1, 3).contiguous()
    t_dev = None if t is None else torch.tensor([t], dtype=torch.float32, device="cuda")
    tk = tvt = tbias = None
    T = Tpad = 0
    if txt is not None:
        tk = txt["k"].contiguous()
        T, Tpad = tk.shape[2], X.pad64(tk.shape[2])
        tvt, tbias = X.make_vt(txt["v"], Tpad), X.make_bias(txt["valid"], T, Tpad, k.device)
    ins = [raw["qkv"], raw["stat"], raw["w"], raw["b"], table, table_t, k, vt, tk, tvt, tbias, gate]
    before = _snapshot(ins)
    guard = Guarded(B * N, H * hd)
    rc = lib().lt_op_attention_qraw_ex(P(raw["qkv"]), raw["ld"], raw["q_col0"], P(raw["stat"]), P(raw["w"]), P(raw["b"]), P(table), P(table_t),
                                       tlen or table.shape[1], grid_w or raw["grid_w"], P(t_dev), WATERSHED, P(k), P(vt), P(tk), P(tvt), P(tbias),
                                       P(gate), T, Tpad, P(guard.out), B, H, Hkv, N, Nkpad, hd, stream())
    torch.cuda.synchronize()
    guard.assert_intact(what)
    _assert_unchanged(ins, before, what)
    if expect_refusal:
        assert rc != 0 and bool(torch.isnan(guard.out.float()).all()), f"{what}: rc {rc}, or the output was touched"
        return None
    ok(rc, what)
    return guard.out.view(B, N, H, hd).permute(0, 2, 1, 3)


def run_small(raw, t, what="", expect_refusal=False, **override):
    """lt_op_attention_small on a guarded NaN-filled output -> bf16 [B, H, N, hd]; override: arguments replaced for the refusal cases"""
    from gpu_util import P, lib, ok, stream
    B, H, Hkv, N, hd = raw["shape"]
    a = dict(tokens=N, hd=hd, k_nslot=raw["k_nslot"], grid_w=raw["grid_w"], table_len=raw["table"].shape[1])
    a.update(override)
    t_dev = None if t is None else torch.tensor([t], dtype=torch.float32, device="cuda")
    ins = [raw["qkv"], raw["rowstat"], raw["qw"], raw["qb"], raw["kw"], raw["kb"], raw["table"]]
    before = _snapshot(ins)
    guard = Guarded(B * N, H * hd)
    rc = lib().lt_op_attention_small(P(raw["qkv"]), raw["ld"], raw["q_col0"], raw["k_col0"], raw["v_col0"], P(raw["rowstat"]), raw["slots"], raw["q_slot0"],
                                     raw["q_nslot"], raw["k_slot0"], a["k_nslot"], P(raw["qw"]), P(raw["qb"]), P(raw["kw"]), P(raw["kb"]), P(raw["table"]),
                                     a["table_len"], a["grid_w"], P(t_dev), WATERSHED, float(raw["k_scale"]), P(guard.out), B, H, Hkv, a["tokens"], a["hd"],
                                     stream())
    torch.cuda.synchronize()
    guard.assert_intact(what)
    _assert_unchanged(ins, before, what)
    if expect_refusal:
        assert rc != 0 and bool(torch.isnan(guard.out.float()).all()), f"{what}: rc {rc}, or the output was touched"
        return None
    ok(rc, what)
    return guard.out.view(B, N, H, hd).permute(0, 2, 1, 3)
