"""Exact-softmax attention checks: generators, the float64 expected value and the word-exact comparator (plain module, no test in here).

The flash-attention recurrence, like the GEMM of tests/exact_operands.py, has inputs on which the kernel's own rounding points add no
error.  In the log2 domain (k_prescaled = 1: scores are plain q . k):
  * q and k hold small integers -> every score is an exact integer in fp32, in any order of the reduction;
  * within one (sample, kv-head) a query row sees every key either at a LEVEL 0, -1, ..., -7 below the row's maximum or OFF, at least
    64 below it -> every weight 2^(s - m) is a power of two, exact in bf16 also under the deferred maximum (THR = 8: P <= 2^8), a
    bf16-pair maximum holds the integer m exactly, and a rescale multiplies O and l by the same power of two;
  * V holds small integers -> P . V and the row sum are exact in fp32 (2^8 * 2^7 * sum_live 2^level |v| < 2^24).
What stays inexact is the final O * rcp(l) and at most an fp32 ulp in exp2 / the fp32 row sum: a float64 value x that lies further than
relative DELTA from a bf16 rounding midpoint has ONE correct output word, RN_bf16(x); within DELTA either neighbour is accepted (and still
compared).  The share of such words is capped per call (MAX_AMBIGUOUS) as a condition on the inputs.

Two families: `selector` (one live key per row: the output is that key's V row, bit for bit, and a wrong word names where it came from)
and `levels` (1 to about 1000 live keys per row, levels drawn through a rank-16 integer code, live keys on the first and last key of
every tile and on the last valid key, the row's maximum early, late or in the middle of the key sequence).
`expected()` checks every precondition on every call; a draw that violates one is a PreconditionError, never a looser comparison."""
import ctypes as C
import math

import torch

from exact_operands import Guarded, PreconditionError, _runs

DELTA = 2.0 ** -20        # ~1.5 fp32 ulp for rcp and multiply, times a margin of 5 for exp2 / an fp32 row sum
MAX_AMBIGUOUS = 0.03
OFF = 72                  # score of a gated-off key below a live one at the same level: >= 65 below the row's maximum
NLEVEL = 8
NRHO = 16                 # row classes = rank of the level code
L2E = 1.4426950408889634
SEL_R, SEL_R2, SEL_D, SEL_A = 11, 5, 4, 128   # selector: key index in 4 digits base 11 (14641 keys; the text slot: base 5, 625), one-hot per digit, q = 128 on the row's digits
W_BUDGET = 200.0          # menu rule: estimated sum_live 2^level per row (the precondition itself is checked exactly: < 512)
MEAN_W = 0.142            # mean of 2^-1 .. 2^-7


# ---- integer hashing (the same draw on any device, no RNG state) -------------------------------------------------------------------------
def _mix(x, seed):
    x = (x + (int(seed) * 0x9E3779B1 & 0xFFFFFFFF)) & 0xFFFFFFFF
    x = ((x ^ (x >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
    x = ((x ^ (x >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _ar(n, device):
    return torch.arange(n, device=device, dtype=torch.int64)


def v_position(n):
    """position of key n inside the V^T rows (include/lumina_dit.h: bits 2 and 3 of the key index swapped inside every 16 keys)"""
    return (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)


def _dim_perm(hd, b, kvh, seed, device):
    """where logical dim i of the construction sits among the hd reduction indices of (sample b, kv-head kvh)"""
    return torch.argsort(_mix(_ar(hd, device) * 64 + b * 8 + kvh, seed + 11))


def _filler(nrow, nfill, a, b, seed, device, signed):
    """cancelling pairs: logical dims (i, i + nfill / 2) carry (f, f) on the query side and (g, -g) on the key side: every reduction index
    multiplies non-zero operands, the pair adds nothing to the score"""
    half = nfill // 2
    h = _mix(_ar(nrow, device)[:, None] * 131 + _ar(half, device)[None, :] + a * 7919 + b * 104729, seed)
    mag = (h % 3 + 1).double()
    if not signed:
        return torch.cat([mag, mag], 1)
    g = mag * (1 - 2 * ((h >> 8) & 1)).double()
    return torch.cat([g, -g], 1)


def _valid_list(B, Nk, valid):
    valid = [Nk] * B if valid is None else list(valid)
    assert len(valid) == B and all(1 <= n <= Nk for n in valid), (valid, Nk)
    return valid


# ---- generators -------------------------------------------------------------------------------------------------------------------------
def selector(B, H, Hkv, N, Nk, hd, seed=0, valid=None, device="cpu", slot=0, nslots=1, kseed=None):
    """one live key per query row: q . k = 128 (2 * matching digits - 4) in {-512, ..., 512}: 512 for the selected key, <= 256 for every
    other; v[b, kvh, key, d] = +-(1 + (7 key + 13 d + 29 kvh + 3 b) % 255).  slot / nslots: see levels()."""
    R = (SEL_R, SEL_R2)[slot]
    base, ng, nfix = (0, SEL_R * SEL_D)[slot], R * SEL_D, SEL_R * SEL_D + (SEL_R2 * SEL_D if nslots == 2 else 0)
    assert Nk <= R ** SEL_D and hd >= nfix + 4 and (hd - nfix) % 2 == 0 and H % Hkv == 0
    kseed = seed if kseed is None else kseed
    valid, rep = _valid_list(B, Nk, valid), H // Hkv
    q = torch.zeros(B, H, N, hd, dtype=torch.float64, device=device)
    k = torch.zeros(B, Hkv, Nk, hd, dtype=torch.float64, device=device)
    v = torch.zeros(B, Hkv, Nk, hd, dtype=torch.float64, device=device)
    sel = torch.zeros(B, H, N, dtype=torch.int64, device=device)
    j, r, d = _ar(Nk, device), _ar(N, device), _ar(hd, device)
    digit_of = lambda idx: torch.stack([(idx // R ** t) % R + R * t for t in range(SEL_D)], -1)  # logical dim of each digit (from base)
    for b in range(B):
        for kvh in range(Hkv):
            perm = _dim_perm(hd, b, kvh, seed, device)
            kl = torch.zeros(Nk, hd, dtype=torch.float64, device=device)
            kl[:, base:base + ng] = -1.0
            kl[:, nfix:] = _filler(Nk, hd - nfix, b, kvh, kseed + 1, device, True)
            kl[:, base:base + ng].scatter_(1, digit_of(j), 1.0)
            k[b, kvh][:, perm] = kl
            sign = 1 - 2 * (_mix(j[:, None] * 257 + d[None, :] + 65537 * (b * Hkv + kvh), kseed + 2) & 1)
            v[b, kvh] = (sign * (1 + (7 * j[:, None] + 13 * d[None, :] + 29 * kvh + 3 * b) % 255)).double()
            for h in range(kvh * rep, (kvh + 1) * rep):
                s = (r * 37 + 101 * h + 17 * b + 3 + kseed) % valid[b]
                ql = torch.zeros(N, hd, dtype=torch.float64, device=device)
                if slot == 0:
                    ql[:, nfix:] = _filler(N, hd - nfix, b, h + 64, seed + 3, device, False)
                ql[:, base:base + ng].scatter_(1, digit_of(s), float(SEL_A))
                q[b, h][:, perm] = ql
                sel[b, h] = s
    return dict(family="selector", q=q.to(torch.bfloat16), k=k.to(torch.bfloat16), v=v.to(torch.bfloat16), valid=valid, sel=sel)


_P_MENU = [(0, 0, 1.0), (1, 0, 9.0), (0, 1, 55.0), (1, 1, 63.0)]   # (mid-small live, mid-large live, live keys per 64-key tile ~)
SLOT = 24


def levels(B, H, Hkv, N, Nk, hd, seed=0, valid=None, device="cpu", slot=0, nslots=1, kseed=None):
    """logical reduction dims of a slot (24 of them): 0-3 position class of the key (first of a tile | last of a tile or last valid key |
    1/8 of the others | the rest), 4-7 tile class ((tile + b + kvh) % 4), 8-23 the level code y[key][rho] in 0..7 (the query holds -1
    at its row class rho); behind the slots: cancelling pairs.  A gate dim holds +1 on the query side where the row keeps the class and
    -OFF where it drops it; the first / last classes and the tile class of the row's own maximum tile are always kept, so every row
    has a live valid key.  nslots = 2 (the fused self + text launch, one query tensor for two key sets): the self keys live in slot 0,
    the text keys in slot 1, each zero in the other's dims; the slot-1 draw returns only its own query dims, to be ADDED to slot 0's."""
    nfix, base = SLOT * nslots, SLOT * slot
    assert hd >= nfix + 4 and (hd - nfix) % 2 == 0 and H % Hkv == 0
    kseed = seed if kseed is None else kseed
    valid, rep = _valid_list(B, Nk, valid), H // Hkv
    q = torch.zeros(B, H, N, hd, dtype=torch.float64, device=device)
    k = torch.zeros(B, Hkv, Nk, hd, dtype=torch.float64, device=device)
    v = torch.zeros(B, Hkv, Nk, hd, dtype=torch.float64, device=device)
    j, r, d, rho_all, four = _ar(Nk, device), _ar(N, device), _ar(hd, device), _ar(NRHO, device), _ar(4, device)
    tile, pos = j // 64, j % 64
    for b in range(B):
        ntl = (valid[b] + 63) // 64
        ntc = min(4, ntl)
        tstar = ((rho_all * ntl) // NRHO + rho_all) % ntl                                   # the tile of row class rho's maximum
        menu = [(ms, ml, w) for ms, ml, kpt in _P_MENU for w in (1, 2, 4) if w <= ntc and kpt * ntl * min(w + 1, ntc) / ntc * MEAN_W <= W_BUDGET]   # (+ 1: the maximum tile's class)
        menu_t = torch.tensor(menu, device=device, dtype=torch.int64)
        for kvh in range(Hkv):
            perm = _dim_perm(hd, b, kvh, seed, device)
            hk = _mix(j * 8191 + 65537 * (b * Hkv + kvh), kseed + 4)
            pc = torch.where((pos == 63) | (j == valid[b] - 1), 1, torch.where(pos == 0, 0, torch.where(hk % 8 == 0, 2, 3)))
            tc = (tile + b + kvh) % ntc
            kg = torch.zeros(Nk, SLOT, dtype=torch.float64, device=device)
            kg[:, 4 + ntc:8] = 1.0                                             # tile classes that hold no key: a constant on every key
            kg[:, 0:4].scatter_(1, pc[:, None], 1.0)
            kg[:, 4:8].scatter_(1, tc[:, None], 1.0)
            hy = _mix(j[:, None] * NRHO + rho_all[None, :] + 1048583 * (b * Hkv + kvh), kseed + 5)
            at_star = tile[:, None] == tstar[None, :]
            y = torch.where(at_star, hy % NLEVEL, 1 + hy % (NLEVEL - 1))
            y = torch.where(at_star & (pc[:, None] <= 1), 0, y)                # the maximum sits on the edge keys of tile tstar
            kg[:, 8:24] = y.double()
            kl = torch.zeros(Nk, hd, dtype=torch.float64, device=device)
            kl[:, base:base + SLOT] = kg
            kl[:, nfix:] = _filler(Nk, hd - nfix, b, kvh, kseed + 1, device, True)
            k[b, kvh][:, perm] = kl
            hv = _mix(j[:, None] * 257 + d[None, :] + 65537 * (b * Hkv + kvh), kseed + 2)
            sign = 1 - 2 * (_mix(d + 257 * (b * Hkv + kvh), kseed + 7) & 1)
            v[b, kvh] = ((1 + (hv & 1)) * sign[None, :]).double()   # 1 or 2, one sign per column: the live keys of a word cannot cancel
            for h in range(kvh * rep, (kvh + 1) * rep):
                hr = _mix(r * 31 + 1009 * h + 9176 * b, kseed + 6)
                rho = (r + 3 * h + 5 * b) % NRHO
                m = menu_t[hr % len(menu)]
                t0 = (hr >> 8) % ntc
                keep_t = ((four[None, :] - t0[:, None]) % ntc) < m[:, 2:3]                       # [N, 4]
                keep_t |= four[None, :] == ((tstar[rho] + b + kvh) % ntc)[:, None]
                keep_t[:, ntc:] = True
                keep_p = torch.cat([torch.ones(N, 2, dtype=torch.bool, device=device), m[:, 0:1] > 0, m[:, 1:2] > 0], 1)
                qg = torch.zeros(N, SLOT, dtype=torch.float64, device=device)
                qg[:, 0:4] = torch.where(keep_p, 1.0, -float(OFF))
                qg[:, 4:8] = torch.where(keep_t, 1.0, -float(OFF))
                qg[:, 8:24].scatter_(1, rho[:, None], -1.0)
                ql = torch.zeros(N, hd, dtype=torch.float64, device=device)
                ql[:, base:base + SLOT] = qg
                if slot == 0:
                    ql[:, nfix:] = _filler(N, hd - nfix, b, h + 64, seed + 3, device, False)
                q[b, h][:, perm] = ql
    return dict(family="levels", q=q.to(torch.bfloat16), k=k.to(torch.bfloat16), v=v.to(torch.bfloat16), valid=valid)


GENERATORS = {"selector": selector, "levels": levels}


def every_reduction_index_is_used(inp):
    """in every whole 64-row block of every head each of the hd reduction indices multiplies a non-zero q by a non-zero k for some
    (row, valid key)"""
    q, k = inp["q"], inp["k"]
    B, H, N, hd = q.shape
    rep = H // k.shape[1]
    for b in range(B):
        kn = (k[b, :, :inp["valid"][b]] != 0).any(1)                                   # [Hkv, hd]
        if N >= 64:
            qn = (q[b, :, :N // 64 * 64] != 0).view(H, N // 64, 64, hd).any(2)         # [H, blocks, hd]
            if not bool((qn & kn.repeat_interleave(rep, 0)[:, None, :]).all()):
                return False
    return True


# ---- expected value ----------------------------------------------------------------------------------------------------------------------
def _is_int(t):
    return bool((t == t.round()).all())


def expected(inp, k_prescaled=1, scale=1.0, row_chunk=1024):
    """float64 base-2 softmax attention over all keys (off keys included; masked keys: -inf), [B, H, N, hd] on the inputs' device, one
    (b, h) and row chunk at a time, after the precondition checks of the module docstring.  k_prescaled = 0 (selector only): scores are
    q . k * scale * log2(e)."""
    q, k, v, valid, fam = inp["q"], inp["k"], inp["v"], inp["valid"], inp["family"]
    B, H, N, hd = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    rep = H // Hkv
    if not (_is_int(q.double()) and _is_int(k.double()) and _is_int(v.double())):
        raise PreconditionError("q, k and v must hold integers")
    if not hd * float(q.double().abs().max()) * float(k.double().abs().max()) < 2 ** 24:
        raise PreconditionError("sum |q| |k| can reach 2^24: a score could round in fp32")
    if fam == "levels" and not k_prescaled:
        raise PreconditionError("the levels family needs k_prescaled = 1: a scale makes the weights inexact")
    out = torch.empty(B, H, N, hd, dtype=torch.float64, device=q.device)
    jj = _ar(Nk, q.device)
    stats = dict(max_live=0, min_live=Nk, jump=0, small_raise=0, rows=0)
    for b in range(B):
        masked = jj >= valid[b]
        for h in range(H):
            kd, vd = k[b, h // rep].double(), v[b, h // rep].double()
            for r0 in range(0, N, row_chunk):
                s = q[b, h, r0:r0 + row_chunk].double() @ kd.t()
                if float(s.abs().max()) > 512:
                    raise PreconditionError(f"|q . k| reaches {float(s.abs().max())} > 512")
                s = s.masked_fill(masked[None, :], float("-inf"))
                m = s.max(1, keepdim=True).values
                rel = s - m                                                # integers (or -inf)
                live, off = rel >= -(NLEVEL - 1), rel <= -64
                if fam == "selector":
                    if not bool((live.sum(1) == 1).all() and (rel[~live] <= -256).all()):
                        raise PreconditionError("selector: a row without exactly one key 256 above all others")
                    if not torch.equal(s.argmax(1), inp["sel"][b, h, r0:r0 + row_chunk]):
                        raise PreconditionError("selector: the live key is not the selected one")
                    w = torch.exp2(rel * (1.0 if k_prescaled else scale * L2E))
                else:
                    if not bool((live | off).all()):
                        raise PreconditionError("levels: a key neither at a level 0..-7 nor >= 64 below the row's maximum")
                    w = torch.exp2(rel)
                    wl = w * live
                    if not bool(((w * off).sum(1) < 2.0 ** -28 * w.sum(1)).all()):
                        raise PreconditionError("levels: the off keys weigh more than 2^-28 of a row sum")
                    if not bool(((w * off) @ vd.abs() <= 2.0 ** -26 * (wl @ vd).abs()).all()):
                        raise PreconditionError("levels: a word whose live keys cancel: the off keys would decide it")
                    worst = max(float(wl.sum(1).max()), float((wl @ vd.abs()).max()))
                    if not 2.0 ** 15 * worst < 2.0 ** 24:
                        raise PreconditionError(f"levels: sum_live 2^level |v| = {worst} >= 512: P . V or the row sum could round in fp32")
                    # coverage figures (64-key tiles in sequence): rows whose running maximum jumps by more than THR = 8 / rises by less
                    nt = (Nk + 63) // 64
                    sp = torch.nn.functional.pad(s, (0, nt * 64 - Nk), value=float("-inf")).view(s.shape[0], nt, 64).max(2).values
                    run = torch.cummax(sp, 1).values
                    step = run[:, 1:] - run[:, :-1]
                    stats["jump"] += int((step > 8).any(1).sum())
                    stats["small_raise"] += int(((step > 0) & (step <= 8)).any(1).sum())
                nlive = live.sum(1)
                stats["max_live"], stats["min_live"] = max(stats["max_live"], int(nlive.max())), min(stats["min_live"], int(nlive.min()))
                stats["rows"] += s.shape[0]
                out[b, h, r0:r0 + row_chunk] = (w @ vd) / w.sum(1, keepdim=True)
    inp["stats"] = stats
    if fam == "selector":
        want = torch.stack([v[b].double()[torch.arange(H, device=q.device)[:, None] // rep, inp["sel"][b]] for b in range(B)])
        if not bool(((out - want).abs() <= 2.0 ** -12 * want.abs()).all() and (want != 0).all()):
            raise PreconditionError("selector: the float64 softmax is not within 2^-12 of the selected V row")
    return out


# ---- comparator --------------------------------------------------------------------------------------------------------------------------
def neighbours(x, delta=DELTA):
    """(rn, lo, hi, ambiguous) of float64 x: the bf16 neighbours below / above |x| (sign restored; lo = hi = rn = 0 at 0), round-to-nearest-even
    and whether x lies within relative delta of the midpoint.  All three are exact in bf16 and returned as float32."""
    mant, e = torch.frexp(x.abs())
    t = mant * 256.0                                   # [128, 256): one bf16 ulp = 1
    fl = torch.floor(t)
    frac = t - fl
    ulp = torch.ldexp(torch.ones_like(x), e - 8)
    sign = torch.sign(x)
    lo, hi = sign * fl * ulp, sign * (fl + 1) * ulp
    up = (frac > 0.5) | ((frac == 0.5) & (fl % 2 == 1))
    rn = torch.where(up, hi, lo)
    amb = ((frac - 0.5).abs() <= delta * t) & (x != 0)
    return rn.float(), lo.float(), hi.float(), amb


def _r16(t):
    return t.to(torch.bfloat16).float()


def admissible(parts, combine, delta=DELTA):
    """parts: float64 tensors (the softmax outputs that feed one output word); combine(*bf16-valued fp32 tensors) -> fp32 of bf16 values:
    the later rounding points, exact fp32 operations on bf16 values.  Returns (want, [every admissible word], ambiguous): want uses RN of
    every part, the list runs both neighbours of every ambiguous part through `combine`."""
    nb = [neighbours(p, delta) for p in parts]
    want = combine(*[n[0] for n in nb])
    amb = torch.zeros_like(nb[0][3])
    for n in nb:
        amb |= n[3]
    cands = []
    for mask in range(1 << len(parts)):
        for mask2 in range(1 << len(parts)):
            pick = []
            for i, n in enumerate(nb):
                alt = n[2] if (mask2 >> i) & 1 else n[1]
                pick.append(torch.where(n[3], alt, n[0]) if (mask >> i) & 1 else n[0])
            if mask2 & ~mask:
                continue
            cands.append(combine(*pick))
    return want, cands, amb


def assert_attention_words(got, parts, combine=lambda o: o, what="", delta=DELTA, inp=None):
    """every word of got (bf16 [B, H, N, hd]) must be the one correct word (see module docstring).  Returns the ambiguous share.  The
    failure message groups the wrong words by (b, h, 64-row block, 16-column range)."""
    assert got.dtype == torch.bfloat16 and got.shape == parts[0].shape, (got.dtype, got.shape, parts[0].shape)
    want, cands, amb = admissible(parts, combine, delta)
    share = float(amb.double().mean())
    if share > MAX_AMBIGUOUS:
        raise PreconditionError(f"{what}: {share:.2%} of the words lie within 2^{math.log2(delta):.0f} of a bf16 midpoint (cap {MAX_AMBIGUOUS:.0%})")
    g = got.float()
    good = g == want
    for c in cands:
        good |= amb & (g == c)
    bad = ~good
    n = int(bad.sum())
    if n == 0:
        return share
    idx = bad.nonzero()
    B, H, N, hd = got.shape
    key = ((idx[:, 0] * H + idx[:, 1]) * ((N + 63) // 64) + idx[:, 2] // 64) * ((hd + 15) // 16) + idx[:, 3] // 16
    groups, counts = torch.unique(key, return_counts=True)
    order = torch.argsort(counts, descending=True)[:8]
    glist = []
    for gi in order.tolist():
        kk = int(groups[gi])
        dr, kk = kk % ((hd + 15) // 16), kk // ((hd + 15) // 16)
        rb, kk = kk % ((N + 63) // 64), kk // ((N + 63) // 64)
        glist.append(f"(b {kk // H}, h {kk % H}, rows {rb * 64}-{min(N, rb * 64 + 64) - 1}, cols {dr * 16}-{min(hd, dr * 16 + 16) - 1}): {int(counts[gi])}")
    first = []
    for b, h, r, d in idx[:4].tolist():
        item = f"(b {b}, h {h}, row {r}, col {d}: got {float(g[b, h, r, d])}, want {float(want[b, h, r, d])}, float64 {float(parts[0][b, h, r, d]):.9g})"
        if inp is not None and inp["family"] == "selector" and len(parts) == 1:
            item += " " + _selector_source(inp, b, h, d, float(g[b, h, r, d]))
        first.append(item)
    nan = int(torch.isnan(g)[bad].sum())
    hr = torch.bincount(idx[:, 2] % 256, minlength=256).cpu()
    raise AssertionError(f"{what}: {n} of {bad.numel()} words wrong ({nan} unwritten / NaN, {int((bad & amb).sum())} of them ambiguous words outside "
                         f"both neighbours; ambiguous share {share:.3%}); {len(groups)} (b, h, 64-row block, 16-col range) groups, largest: "
                         + "; ".join(glist) + "; first: " + "; ".join(first) + f"; by row % 256 {_runs(hr)}")


def _selector_source(inp, b, h, d, value):
    """where in V a wrong selector word came from: the same column of any kv-head first, then any column"""
    v = inp["v"][b].float()
    rep = inp["q"].shape[1] // v.shape[0]
    hit = (v[:, :, d] == value).nonzero()
    if hit.numel():
        return "[= v of " + ", ".join(f"(kvh {a}, key {j})" for a, j in hit[:3].tolist()) + f" at this column; own kvh {h // rep}]"
    hit = (v == value).nonzero()
    if hit.numel():
        return "[= v of " + ", ".join(f"(kvh {a}, key {j}, col {c})" for a, j, c in hit[:3].tolist()) + "]"
    return "[no V word has this value]"


def gated(prev, gate_bf16):
    """combine() of lt_op_attention's accumulate mode: R(prev + R(o * bf16(tanh(g)))); prev fp32 [B, H, N, hd], gate bf16 [H]"""
    gt = _r16(torch.tanh(gate_bf16.float())).view(1, -1, 1, 1)
    return lambda o: _r16(prev + _r16(o * gt))


def fused(gate_bf16):
    """combine() of lt_op_attention_fused: R(R(o_self) + R(R(o_txt) * bf16(tanh(g))))"""
    gt = _r16(torch.tanh(gate_bf16.float())).view(1, -1, 1, 1)
    return lambda o_self, o_txt: _r16(o_self + _r16(o_txt * gt))


def gate_values(H, seed, device="cpu"):
    """bf16 [H] from {+20, -20, 0}: bf16(tanh(g)) is +1, -1 or 0 under any tanh implementation; every value occurs from H = 3 on"""
    return (torch.tensor([20.0, -20.0, 0.0], device=device)[(_ar(H, device) + seed) % 3]).to(torch.bfloat16)


def small_int_prev(B, H, N, hd, seed, device="cpu"):
    """previous output of the accumulate mode: integers in -8..8, fp32 [B, H, N, hd]"""
    i = _ar(B * H * N * hd, device)
    return (_mix(i, seed + 9) % 17 - 8).float().view(B, H, N, hd)


# ---- operands in the kernels' layouts and the launches ----------------------------------------------------------------------------------
def make_vt(v, Nkpad):
    """[B, Hkv, Nk, hd] -> the V^T image [B, Hkv, hd, Nkpad] of lt_op_v_transpose, built here (keys >= Nk zero)"""
    B, Hkv, Nk, hd = v.shape
    vt = torch.zeros(B, Hkv, hd, Nkpad, dtype=v.dtype, device=v.device)
    vt[..., v_position(_ar(Nk, v.device))] = v.transpose(2, 3)
    return vt.contiguous()


def make_bias(valid, Nk, Nkpad, device):
    """float [B, Nkpad]: 0 on the valid keys, -inf behind them and in the padding"""
    bias = torch.full((len(valid), Nkpad), float("-inf"), dtype=torch.float32, device=device)
    for b, n in enumerate(valid):
        bias[b, :n] = 0.0
    return bias


def pad64(n):
    return (n + 63) // 64 * 64


def describe(B, H, Hkv, N, Nk, hd, bias=False, accumulate=False):
    from gpu_util import lib, ok
    buf = C.create_string_buffer(64)
    ok(lib().lt_op_attention_describe(int(bias), int(accumulate), B, H, Hkv, N, Nk, pad64(Nk), hd, buf, 64))
    return buf.value.decode()


def _finish(guard, B, H, N, hd, what):
    torch.cuda.synchronize()
    guard.assert_intact(what)
    return guard.out.view(B, N, H, hd).permute(0, 2, 1, 3)


def run_attention(inp, use_bias=False, gate=None, prev=None, k_prescaled=1, scale=1.0, what=""):
    """lt_op_attention on a sentinel-guarded, NaN-filled [B * N, H * hd] output (accumulate mode: filled with prev); -> bf16 [B, H, N, hd].
    The guard words (and with them every row >= N of the last sample) must survive; a row < N left unwritten stays NaN and fails the
    comparison."""
    from gpu_util import P, lib, ok, stream
    q, k = inp["q"].contiguous(), inp["k"].contiguous()
    B, H, N, hd = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    Nkpad = pad64(Nk)
    vt = make_vt(inp["v"], Nkpad)
    bias = make_bias(inp["valid"], Nk, Nkpad, q.device) if use_bias else None
    assert use_bias or all(n == Nk for n in inp["valid"]), "a short valid length needs the key bias"
    guard = Guarded(B * N, H * hd)
    if prev is not None:
        guard.out.copy_(prev.permute(0, 2, 1, 3).reshape(B * N, H * hd).to(torch.bfloat16))
    ok(lib().lt_op_attention(P(q), P(k), P(vt), P(bias), P(guard.out), P(gate), 1 if gate is not None else 0, B, H, Hkv, N, Nk, Nkpad, hd,
                             float(scale), int(k_prescaled), stream()), "attention")
    return _finish(guard, B, H, N, hd, what)


def run_attention_fused(inp, txt, gate, what=""):
    """lt_op_attention_fused: inp the self-attention operands, txt a second draw over the SAME queries (its q is inp's q)"""
    from gpu_util import P, lib, ok, stream
    q, k = inp["q"].contiguous(), inp["k"].contiguous()
    tk = txt["k"].contiguous()
    B, H, N, hd = q.shape
    Hkv, Nk, T = k.shape[1], k.shape[2], tk.shape[2]
    Nkpad, Tpad = pad64(Nk), pad64(T)
    vt, tvt = make_vt(inp["v"], Nkpad), make_vt(txt["v"], Tpad)
    tbias = make_bias(txt["valid"], T, Tpad, q.device)
    guard = Guarded(B * N, H * hd)
    ok(lib().lt_op_attention_fused(P(q), P(k), P(vt), P(tk), P(tvt), P(tbias), P(gate), P(guard.out), B, H, Hkv, N, Nk, Nkpad, T, Tpad, hd,
                                   stream()), "attention_fused")
    return _finish(guard, B, H, N, hd, what)


def fused_draw(family, B, H, Hkv, N, T, hd, seed, valid, device):
    """(self operands, text operands) of one fused launch: two draws in two slots of the reduction dims, ONE query tensor (the sum of the
    two draws' query dims), which both returned dicts carry - each side's preconditions are checked against it"""
    a = GENERATORS[family](B, H, Hkv, N, N, hd, seed=seed, device=device, slot=0, nslots=2)
    t = GENERATORS[family](B, H, Hkv, N, T, hd, seed=seed, valid=valid, device=device, slot=1, nslots=2, kseed=seed + 100)
    a["q"] = t["q"] = (a["q"].float() + t["q"].float()).to(torch.bfloat16)
    return a, t
