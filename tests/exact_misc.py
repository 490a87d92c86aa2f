"""Boundary-kernel checks (the kernels of csrc/misc.hip and the stand-alone router of csrc/moe.hip): references, input generators and comparators
(plain module, no test in here).  Built from exact_rows.Chain, exact_attention.neighbours / MAX_AMBIGUOUS and exact_operands' quantum precondition.

Four classes of kernel:
  a. movement (patchify at a bf16 source, eol_fill, fill_rows, label_gather, mask_to_bias, the bf16 paths of cast / upload_rows): the output words
     are an index computation in numpy written from the reference lines each function cites; sources are random 16-bit patterns (NaN, denormals
     included), outputs are compared as integers, words the kernel must not touch keep the sentinel.
  b. conversions (fp32 / f16 sources): ONE correct word by integer arithmetic on the bits (round to nearest even), cross-checked against torch's
     CPU cast; a NaN input asks for a NaN output with any payload.
  c. rounding chains in float64, stage by stage (exact_rows.Chain): a bf16 x bf16 product is exact in fp32, a two-term sum carries one fp32 rounding (U)
     where fp32 does not hold it exactly, a product with an fp32 scalar is evaluated with its one fp32 rounding (float64 holds it exactly), tanh
     takes DELTA_TANH.  A word whose float64 pre-image lies
     within the stage bound of a bf16 midpoint is ambiguous: both neighbours are carried on, the output must equal one candidate, and the share
     of such words is capped per call (MAX_AMBIGUOUS) as a condition on the draw (PreconditionError), never a looser comparison.
     The fp32 ODE state has no bound at all: numpy float32, operation by operation, exactly as torch evaluates the solver's expressions.
  d. linear_small_m beyond the identity case: operands for which the dot product is exact in fp32 in any order, with the activated / summed /
     generated inputs known word for word, and prep_mod's chain on the rounded output.

Bounds that rest on documented rather than measured accuracy (this project has NOT measured the device library on gfx950; words outside these
bounds on the GPU are a finding).  One ulp of an fp32 result is at most 2 U of its magnitude (U = 2^-24):
  expf <= 3 ulp, sinf / cosf <= 4 ulp, powf <= 16 ulp, rsqrtf <= 2 ulp, tanhf <= 5 ulp: the OpenCL full-profile figures the ROCm device libraries
  are built to (the same source exact_rows.py uses for tanh); the fp32 division is IEEE (correctly rounded), as hipcc compiles it by default.
timestep_features, per word (operation count):  x = (c k) / half: two roundings, |dx| <= 2 U |x|;  f = expf(x): df / f <= |dx| + 6 U;
  arg = t f: one more U;  cos / sin: |d value| <= |d arg| + 8 U |value|.  TS bound = MARGIN (arg (2 |x| + 7) U + 8 U |value|), MARGIN = 4 as in
  exact_rows.py.  t stays in [0, 1] (the engine passes nothing else; beyond that the argument error outgrows a bf16 spacing).
rope_table, per word:  e = (step fi) / hd: U;  powf(theta, e): ln(theta) e U + 32 U;  1 / .: U;  two more operations (a division and a product, in
  either order): 2 U;  so d ang / ang <= (ln(theta) e + 36) U, and cos / sin add 8 U |value|.  ROPE bound = MARGIN (|ang| (ln(theta) e + 36) U + 8 U |value|).
cap_pool_ln: the pooled vector is known exactly (quantum precondition: every partial sum over T is exact; one IEEE division; one bf16 rounding
  at a bf16 source).  LayerNorm statistics, this kernel's reduction order: ceil(C / 256) serial adds per thread, the wave butterfly (6), the four
  partials (3), / C (1): mean error <= (ceil(C / 256) + 10) U mean|x|; the variance the same chain over (x - mean)^2 (two more roundings per
  term), + eps (1), rsqrtf 2 ulp: rstd error <= ((ceil(C / 256) + 13) / 2 + 4) U relative.  Margin 4; per word assembled as exact_rows' LayerNorm."""
import math

import numpy as np
import torch

import exact_rows as R
from exact_attention import MAX_AMBIGUOUS, neighbours
from exact_operands import SENTINEL, SILU_MIN_MARGIN_FP32_ULP, PreconditionError, _quantum, silu_margins
from exact_rows import DELTA_TANH, MARGIN, Chain, U, d64, f32, rn

FP32_EXACT = float(1 << 24)
SENT16 = int(torch.tensor(SENTINEL, dtype=torch.bfloat16).view(torch.int16))        # the bf16 word of 7.0
SENT32F = int(torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32))
LN1E4 = f32(-9.210340371976184)                                                      # -ln(1e4) as the fp32 tensor expression sees it
THIRD = np.float32(1.0) / np.float32(3.0)


# ---- guarded buffers ------------------------------------------------------------------------------------------------------------------------
def guarded(n, dtype=torch.bfloat16, device="cuda"):
    """n words of SENTINEL (7) between guard zones of the same value: a written word is told from an untouched one by the expected image"""
    return R.GuardedBuf(n, device=device, dtype=dtype, fill=SENTINEL)


def sentinel_like(shape, dtype=np.int16):
    return np.full(shape, {np.int16: SENT16, np.int32: SENT32F}[dtype], dtype=dtype)


def bits(t):
    """integer view of a tensor's words as numpy (bf16 / f16 -> int16, fp32 / int32 -> int32)"""
    t = t.detach().cpu().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy()
    return t.numpy()


def random_words(shape, seed):
    """bf16 tensor of random 16-bit patterns over the whole range (NaN, inf, denormal patterns included)"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-32768, 32768, tuple(shape), generator=g, dtype=torch.int32).to(torch.int16)
    return w.view(torch.bfloat16)


def is_nan16(w):
    w = w.astype(np.int64) & 0xFFFF
    return ((w & 0x7F80) == 0x7F80) & ((w & 0x007F) != 0)


def assert_bits(got, want, what, nan_ok=None):
    """integer equality of every word; nan_ok: bool mask of words that must be a bf16 NaN of any payload.  Locates the first wrong words."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    if nan_ok is not None:
        bad = np.where(nan_ok, ~is_nan16(got), bad)
    n = int(bad.sum())
    if n:
        idx = np.argwhere(bad)
        first = [(tuple(int(v) for v in i), hex(int(got[tuple(i)]) & 0xFFFFFFFF), hex(int(want[tuple(i)]) & 0xFFFFFFFF)) for i in idx[:6]]
        untouched = int((got[bad] == (SENT16 if got.dtype == np.int16 else SENT32F)).sum())
        raise AssertionError(f"{what}: {n} of {bad.size} words wrong ({untouched} still hold the sentinel); index range {idx.min(0).tolist()}..{idx.max(0).tolist()}; "
                             f"first (index, got, want): {first}")


# ---- b. conversions -------------------------------------------------------------------------------------------------------------------------
def f32_bits_to_bf16(u, fault=None):
    """round to nearest even on the bits of fp32 words (uint32 numpy) -> (int16 words, NaN mask).  fault 'truncate': the low half dropped"""
    u = u.astype(np.uint64) & 0xFFFFFFFF
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    r = (u >> 16) if fault == "truncate" else ((u + 0x7FFF + ((u >> 16) & 1)) >> 16)
    r = np.where(nan, 0x7FC0, r) & 0xFFFF
    return r.astype(np.uint16).view(np.int16), nan


def convert_words(src, fault=None):
    """(bf16 words int16, NaN mask) of a tensor of dtype fp32 / bf16 / f16, element for element; bf16 is a copy (no NaN mask: words move).
    The integer result is cross-checked against torch's CPU cast on every call."""
    src = src.detach().cpu().contiguous()
    if src.dtype == torch.bfloat16:
        return bits(src), None
    as32 = src.float()                                       # f16 -> fp32 is exact
    want, nan = f32_bits_to_bf16(as32.view(torch.int32).numpy().view(np.uint32), fault)
    if fault is None:
        t = bits(as32.to(torch.bfloat16))
        if not np.array_equal(np.where(nan, 0, t), np.where(nan, 0, want)) or not bool(is_nan16(t)[nan].all()):
            raise PreconditionError("integer round-to-nearest-even and torch's CPU cast disagree")
    return want, nan


def special_f32(n, seed):
    """fp32 inputs of the conversions: random bit patterns, then (cycled) exact ties of both parities and their fp32 neighbours, bf16 denormals,
    +-0, +-inf, the largest finite values (they round up to inf), NaNs"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.randint(0, 1 << 16, (n,), generator=g, dtype=torch.int64)
    hi = torch.randint(0, 1 << 16, (n,), generator=g, dtype=torch.int64)
    u = ((hi << 16) | lo).numpy().astype(np.uint64)
    sp = []
    for base in (0x3F800000, 0x3F810000, 0xC0490000, 0x00010000, 0x00020000, 0x807F0000, 0x7F7F0000, 0xFF7F0000, 0x00000000):
        for low in (0x8000, 0x7FFF, 0x8001, 0x0000, 0xFFFF, 0x0001):     # tie (base even / odd by its bit 16), its neighbours, exact, just below the next
            sp.append(base | low)
    sp += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7FBF8000, 0x00008000, 0x00000001]
    sp = np.array(sp, dtype=np.uint64)
    k = min(n, 4 * len(sp))
    pos = np.arange(k) * max(n // k, 1) % n
    u[pos] = sp[np.arange(k) % len(sp)]
    return torch.from_numpy(u.astype(np.uint32).view(np.int32).copy()).view(torch.float32)


def special_f16(n, seed):
    """every kind of f16 word: random patterns (denormals, inf, NaN included)"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16)
    return w.view(torch.float16)


def source(dtype_code, n, seed):
    """dtype code of the C ABI (0 fp32, 1 bf16, 2 f16) -> a flat source tensor of n words"""
    return (special_f32, lambda n_, s_: random_words((n_,), s_), special_f16)[dtype_code](n, seed)


# ---- a. movement ----------------------------------------------------------------------------------------------------------------------------
def ref_patchify(xw, patch, kpad, dup_first_half, wp_stride, fault=None):
    """xw: int16 words [B, C, H, W] (already converted).  model.py:776-777: x.view(B, C, H/p, p, W/p, p).permute(0, 2, 4, 1, 3, 5).flatten(3) -> rows
    (b, i, j), columns (c, ph, pw); zero padded to kpad; combined = cat([half, half]) (model.py:901-902); rows of a latent row wp_stride apart
    (Flag-DiT's eol slot, lumina_t2i/models/model.py:779-786, keeps the sentinel).  -> int16 [B * Hp * wp_stride, kpad]"""
    B, C, H, W = xw.shape
    Hp, Wp = H // patch, W // patch
    if dup_first_half:
        xw = np.concatenate([xw[:B // 2], xw[:B // 2]], 0)
    rows = xw.reshape(B, C, Hp, patch, Wp, patch).transpose(0, 2, 4, 1, 3, 5).reshape(B, Hp, Wp, C * patch * patch)
    wps = wp_stride if wp_stride > 0 else Wp
    out = sentinel_like((B, Hp, wps, kpad))
    out[:, :, :Wp, :] = 0
    out[:, :, :Wp, :C * patch * patch] = rows
    if fault == "eol_not_skipped":                       # rows packed Wp apart although the layout has Wp + 1 slots per latent row
        flat = sentinel_like((B * Hp * wps, kpad))
        flat[:B * Hp * Wp] = out[:, :, :Wp, :].reshape(B * Hp * Wp, kpad)
        return flat
    return out.reshape(B * Hp * wps, kpad)


def ref_eol_fill(xw, eolw, rows_total, Wp):
    """lumina_t2i/models/model.py:779-786: the last token of each latent row is eol_token.  xw int16 [rows_total * (Wp + 1), d] -> the same, filled"""
    d = xw.shape[1]
    out = xw.copy().reshape(rows_total, Wp + 1, d)
    out[:, Wp, :] = eolw
    return out.reshape(-1, d)


def ref_label_gather(tablew, labels, rows):
    """Next-DiT-ImageNet/models/models.py:216-221: embedding_table(labels); labels outside the table are clamped, the null class is the last row"""
    return tablew[np.clip(labels, 0, rows - 1)]


def ref_mask_to_bias(mask, Tpad):
    """additive key bias: 0 on a valid key, -inf on a masked or padded one -> int32 words of fp32 [B, Tpad]"""
    B, T = mask.shape
    out = np.full((B, Tpad), -np.inf, dtype=np.float32)
    out[:, :T][mask != 0] = 0.0
    return out.view(np.int32)


def upload_row_index(rows, r0, row_map, fault=None):
    """destination row of source row r: row_map 0 -> r0 + r; 1 / 2 -> the packed W1 | W3 layout (32-row groups alternate, include/lumina_dit.h):
    (r / 32) 64 + r % 32, + 32 for the W3 half"""
    r = np.arange(rows)
    if row_map == 0:
        return r0 + r
    return (r >> 5) * 64 + (r & 31) + (32 if row_map == 2 and fault != "no_plus_32" else 0)


def ref_upload_rows(srcw, nan, rows, cols, dst_ld, r0, row_map, dst_rows, fault=None):
    """-> (int16 [dst_rows, dst_ld] with the sentinel wherever nothing is written, NaN mask of the same shape)"""
    out, nmask = sentinel_like((dst_rows, dst_ld)), np.zeros((dst_rows, dst_ld), dtype=bool)
    dr = upload_row_index(rows, r0, row_map, fault)
    out[dr, :cols] = srcw.reshape(rows, cols)
    if nan is not None:
        nmask[dr, :cols] = nan.reshape(rows, cols)
    return out, nmask


# ---- c. rounding chains ---------------------------------------------------------------------------------------------------------------------
def chain_add(a, b):
    a, b = d64(a).reshape(1, -1), d64(b).reshape(1, -1)
    return Chain(a.shape).round(lambda _: a + b, sum2=True)


def unpatchify_index(rows, B, C, out_ch, H, W, patch, wp_stride, fault=None):
    """model.py:749-755: x.view(B, H/p, W/p, p, p, C_out).permute(0, 5, 1, 3, 2, 4) -> [B, C_out, H, W], first C channels kept (:859-861); the token of
    (i, j) sits at i wp_stride + j (an eol column is skipped).  rows: [B * Hp * wp_stride, ld] -> [B, C, H, W] of the same dtype"""
    Hp, Wp = H // patch, W // patch
    wps = wp_stride if wp_stride > 0 else Wp
    ld = rows.shape[1]
    if fault == "eol_not_skipped":
        tok = rows.reshape(-1, ld)[:B * Hp * Wp].reshape(B, Hp, Wp, ld)
    else:
        tok = rows.reshape(B, Hp, wps, ld)[:, :, :Wp]
    x = tok[..., :patch * patch * out_ch].reshape(B, Hp, Wp, patch, patch, out_ch)[..., :C]
    return x.permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)


def ref_unpatchify_cfg(rows, B, C, out_ch, H, W, patch, use_cfg, cfg_scale, cfg_channels, wp_stride, fault=None):
    """model.py:908-913 under bf16: half_eps = uncond + cfg_scale * (cond - uncond) on the first cfg_channels channels, each tensor op rounding:
    R(unc + R(s R(cond - unc))); both halves of the batch receive it; the other channels are copied.  -> Chain over [B * C, H * W]"""
    x = unpatchify_index(d64(rows), B, C, out_ch, H, W, patch, wp_stride, fault)
    ch = Chain((B * C, H * W))
    flat = lambda v: v.reshape(B * C, H * W)
    if not use_cfg:
        ch.cands = [flat(x)]
        ch.first = flat(x)
        return ch
    half = B // 2
    cond, unc = torch.cat([x[:half], x[:half]], 0), torch.cat([x[half:], x[half:]], 0)
    if fault == "swap_cond_uncond":
        cond, unc = unc, cond
    s = f32(cfg_scale)
    cond, unc = flat(cond), flat(unc)
    if fault == "no_inner_round":
        ch.round(lambda _: s * (cond - unc), sum2=True)
    else:
        ch.round(lambda _: cond - unc, sum2=True)
        # the product with the fp32 scalar: 24 + 8 significant bits, exact in float64; .float() is the ONE fp32 rounding it takes (to nearest even,
        # as the multiply instruction's) - so the stage has one correct word.  It matters: at s = 4.3 a fortieth of all bf16 mantissas (k = 20 mod 40)
        # puts 4.3 k within fp32(4.3)'s own representation error of a bf16 midpoint, where a relative-U allowance would call 2.5 % of the words ambiguous
        ch.round(lambda c: (s * c).float().double())
    ch.round(lambda c: unc + c, sum2=True)
    on = flat((torch.arange(C) < cfg_channels)[None, :, None, None].expand(B, C, H, W))
    ch.cands = [torch.where(on, c, flat(x)) for c in ch.cands]
    ch.first = torch.where(on, ch.first, flat(x))
    ch.amb &= on
    return ch


def region_index(N, Hp, Wp, h_split, w_split, fault=None):
    """lumina_next_compositional_generation/models/model.py:872-887: cell (i, j) of (Hp / h_split) x (Wp / w_split) tokens switches on caption
    (i + 1) (j + 1) - 1; later cells overwrite nothing (a mask per caption), tokens beyond the last full cell belong to no cell -> int [N], -1: none.
    A token lies in exactly one cell, so at most one regional caption is on for it."""
    reg = np.full((Hp, Wp), -1, dtype=np.int64)
    hps, wps = Hp // h_split, Wp // w_split
    for i in range(h_split):
        for j in range(w_split):
            reg[hps * i:hps * (i + 1), wps * j:wps * (j + 1)] = (i + 1) * (j + 1) - (0 if fault == "no_minus_1" else 1)
    return reg.reshape(-1)[:N]


def ref_region_text_combine(out, txt, gate, Y, N, H, hd, Hp, Wp, h_split, w_split, fault=None):
    """model.py:422-446: output_y * tanh(gate) (bf16), cond = sum over the regional captions (one is on per token: the fp32 sum of one bf16 value
    and zeros is that value), uncond = the last caption; output + output_y (bf16).  -> Chain over [2 * N, H * hd]: R(out + R(txt R(tanh g)))"""
    d = H * hd
    out, txt, gate = d64(out).reshape(2 * N, d), d64(txt).reshape(Y, N, d), d64(gate)
    reg = torch.from_numpy(region_index(N, Hp, Wp, h_split, w_split, fault))
    use = (reg >= 0) & (reg < Y - 1)
    sel = torch.where(use[:, None], txt[reg.clamp(0, Y - 1), torch.arange(N)], torch.zeros(N, d, dtype=torch.float64))
    t = torch.cat([sel, txt[Y - 1]], 0)
    g = gate.repeat_interleave(hd)[None, :].expand(2 * N, d)
    ch = Chain((2 * N, d))
    ch.round(lambda _: torch.tanh(g), rel=DELTA_TANH)
    ch.round(lambda c: t * c)
    ch.round(lambda c: out + c, sum2=True)
    return ch


def ref_ode_combine_bf16(mode, y0, k1, k2, k3, k4, dt, fault=None):
    """misc.hip's header comment (torchdiffeq fixed-grid arithmetic, every tensor op rounding to bf16; dt is a bf16 value):
       0: y0 + R(dt k1)   1: y0 + R(R(dt k1) / 3)   2: y0 + R(dt R(k2 - R(k1 / 3)))   3: y0 + R(dt R(R(k1 - k2) + k3))
       4: y0 + R(R(R(R(k1 + R(3 R(k2 + k3))) + k4) dt) 0.125); the final sum rounds too.  x / 3 is x times fp32(1 / 3): one fp32 rounding."""
    y0, k1, k2, k3, k4 = (None if v is None else d64(v).reshape(1, -1) for v in (y0, k1, k2, k3, k4))
    dt, third = float(dt), float(THIRD)
    assert float(torch.tensor(dt).to(torch.bfloat16)) == dt, "dt must be a bf16 value at a bf16 state"
    ch = Chain(y0.shape)
    if mode == 0:
        ch.round(lambda _: dt * k1)
    elif mode == 1:
        ch.round(lambda _: dt * k1).round(lambda c: c * third, sum2=True)
    elif mode == 2:
        ch.round(lambda _: k1 * third, sum2=True).round(lambda c: k2 - c, sum2=True).round(lambda c: dt * c)
    elif mode == 3:
        ch.round(lambda _: k1 - k2, sum2=True).round(lambda c: c + k3, sum2=True).round(lambda c: dt * c)
    else:
        ch.round(lambda _: k2 + k3, sum2=True).round(lambda c: 3.0 * c).round(lambda c: k1 + c, sum2=True).round(lambda c: c + k4, sum2=True)
        ch.round(lambda c: c * dt).round(lambda c: c * 0.125)
    return ch.round(lambda c: y0 + c, sum2=True)


def ref_ode_combine_f32(mode, y0, k1, k2, k3, k4, dt, fault=None):
    """the fp32 state: torchdiffeq's expressions (fixed_grid.py, rk_common.rk4_alt_step_func) in numpy float32, one operation at a time, nothing
    fused - ONE correct word.  fault 'fma': the product that feeds a sum is not rounded (modes 2 and 4), as a contracted kernel computes it"""
    y0, k1, k2, k3, k4 = (None if v is None else v.detach().cpu().float().numpy().reshape(-1) for v in (y0, k1, k2, k3, k4))
    dt, three, eighth = np.float32(dt), np.float32(3.0), np.float32(0.125)
    fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)     # (exact product, one rounding)
    if mode == 0:
        r = y0 + dt * k1
    elif mode == 1:
        r = y0 + (dt * k1) * THIRD
    elif mode == 2:
        inner = fma(k1, -THIRD, k2) if fault == "fma" else k2 - k1 * THIRD
        r = y0 + dt * inner
    elif mode == 3:
        r = y0 + dt * ((k1 - k2) + k3)
    else:
        s = k2 + k3
        inner = fma(s, three, k1) if fault == "fma" else k1 + three * s
        r = y0 + ((inner + k4) * dt) * eighth
    return r.astype(np.float32)


def ref_timestep_features(t, dim, fault=None):
    """model.py:63-82 (cast to bf16 at :86): [cos(t f_k) | sin(t f_k)], f_k = exp(-ln(1e4) k / half), k < half = dim / 2.  t: float32 tensor [B].
    -> (float64 value [B, dim], absolute bound [B, dim]): the TS bound of the module header"""
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    x = LN1E4 * k / (half - 1 if fault == "half_minus_1" else half)
    arg = t.detach().cpu().double()[:, None] * torch.exp(x)[None, :]
    c, s = torch.cos(arg), torch.sin(arg)
    if fault == "swap_cos_sin_at_k1":
        c, s = c.clone(), s.clone()
        c[:, 1], s[:, 1] = torch.sin(arg[:, 1]), torch.cos(arg[:, 1])
    darg = arg.abs() * (2 * x.abs()[None, :] + 7) * U
    val = torch.cat([c, s], 1)
    err = MARGIN * (torch.cat([darg, darg], 1) + 8 * U * val.abs())
    return val, err


def chain_timestep_features(t, dim, fault=None):
    val, err = ref_timestep_features(t, dim, fault)
    return Chain(val.shape).round_once(val, err)


def ref_rope_table(length, hd, step, theta0, lin0, theta1, lin1, lin_on_pos):
    """precompute_freqs_cis of the sub-projects as 1-D factor tables (lumina_next_t2i/models/model.py:915-963, Next-DiT-ImageNet/models/models.py:
    977-1012, lumina_t2i/models/model.py:924-960): f = theta^(-step fi / hd); angle = pos (f / lin) or (pos / lin) f.
    -> (float64 [2, len, nf, 2] (cos, sin), absolute bound of the same shape): the ROPE bound of the module header"""
    nf = hd // step
    fi = torch.arange(nf, dtype=torch.float64)
    pos = torch.arange(length, dtype=torch.float64)[:, None]
    out, err = torch.empty(2, length, nf, 2, dtype=torch.float64), torch.empty(2, length, nf, 2, dtype=torch.float64)
    for br, (th, lin) in enumerate(((f32(theta0), f32(lin0)), (f32(theta1), f32(lin1)))):
        e = step * fi / hd
        freq = th ** (-e)
        ang = (pos / lin) * freq[None, :] if lin_on_pos else pos * (freq / lin)[None, :]
        dang = ang.abs() * (abs(math.log(th)) * e[None, :] + 36) * U
        for j, v in enumerate((torch.cos(ang), torch.sin(ang))):
            out[br, ..., j] = v
            err[br, ..., j] = MARGIN * (dang + 8 * U * v.abs())
    return out, err


def cap_ln_derived(C):
    """(mean error over mean|x|, relative rstd error) of cap_pool_ln's LayerNorm statistic, unmargined (module header)"""
    nser = (C + 255) // 256
    return (nser + 10) * U, ((nser + 13) / 2 + 4) * U


def pooled_caption(cap, mask, cap_is_bf16, fault=None):
    """model.py:847-849: (cap_feats * mask).sum(1) / mask.sum(1) in fp32, cast to the features' dtype.  cap values are multiples of a quantum such
    that every partial sum over T is exact in fp32 (checked); the quotient is one IEEE fp32 division.  -> float64 [B, C] of fp32 / bf16 values"""
    capd, m = d64(cap), mask.detach().cpu().double()
    q = _quantum(capd, "caption features")
    worst = float((capd.abs() * m[:, :, None]).sum(1).max()) / q
    if not worst < FP32_EXACT:
        raise PreconditionError(f"caption sums reach {worst} quanta >= 2^24: a partial sum over T could round in fp32")
    s = (capd * m[:, :, None]).sum(1)
    cnt = m.sum(1, keepdim=True) if fault != "mean_over_T" else torch.full((cap.shape[0], 1), float(cap.shape[1]), dtype=torch.float64)
    pooled = torch.from_numpy(s.numpy().astype(np.float32) / cnt.numpy().astype(np.float32)).double()
    return rn(pooled) if cap_is_bf16 else pooled


def ref_cap_pool_ln(cap, mask, ln_w, ln_b, cap_is_bf16, fault=None, eps=1e-5):
    """cap_embedder[0] (model.py:703): the affine LayerNorm of the pooled vector in fp32, one rounding to bf16 -> Chain.round_once over [B, C]"""
    x = pooled_caption(cap, mask, cap_is_bf16, fault)
    w, b = d64(ln_w), d64(ln_b)
    mean, rstd, mabs = R.ln_stats(x, eps)
    cm, cr = (MARGIN * v for v in cap_ln_derived(x.shape[1]))
    u = MARGIN * U
    t = (x - mean) * rstd * w
    a = t + b
    e = cm * mabs * rstd * w.abs() + (cr + 3 * u) * t.abs() + u * a.abs()
    return Chain(x.shape).round_once(a, e)


# ---- d. linear_small_m ----------------------------------------------------------------------------------------------------------------------
def exact_linear(A, W, bias=None):
    """float64 A W^T (+ bias) of operands whose every product and partial sum, in any order, is exact in fp32 (the exact_operands precondition:
    integer multiples of power-of-two quanta, max sum |a w| + |bias| below 2^24 quanta; or one nonzero weight per output) -> the exact value
    [M, N]; ONE rounding to bf16 follows"""
    Ad, Wd = d64(A), d64(W)
    Cv, S = Ad @ Wd.t(), Ad.abs() @ Wd.abs().t()
    if bias is None and int((Wd != 0).sum(1).max()) <= 1:      # selector weights: one bf16 x bf16 product per output and zeros - exact whatever the quanta
        return Cv
    unit = _quantum(Ad, "A") * _quantum(Wd, "W")
    if bias is not None:
        bd = d64(bias)
        if bool((bd != 0).any()):
            unit = min(unit, _quantum(bd, "bias"))
        Cv, S = Cv + bd, S + bd.abs()
    worst = float(S.max()) / unit
    if not worst < FP32_EXACT:
        raise PreconditionError(f"max sum_k |a w| = {worst} quanta >= 2^24: a partial sum could round in fp32")
    return Cv


def pow2_weights(N, K, seed, density=0.25, exps=(-2, 2)):
    """bf16 [N, K] in {-1, 0, +1} 2^e, e per row"""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(N, K, generator=g)
    w = (r < density / 2).float() - (r >= 1 - density / 2).float()
    e = torch.randint(exps[0], exps[1] + 1, (N, 1), generator=g).float()
    return (w * torch.exp2(e)).to(torch.bfloat16)


def selector_weights(N, K, seed):
    """column n has one nonzero +-2^e at k = n mod K (N >= 2 K: every k is read by two columns of different lanes' chunks)"""
    assert N >= 2 * K
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(N, K)
    n = torch.arange(N)
    sign = 1.0 - 2.0 * torch.randint(0, 2, (N,), generator=g).float()
    w[n, n % K] = sign * torch.exp2(torch.randint(-3, 4, (N,), generator=g).float())
    return w.to(torch.bfloat16)


def silu_safe_values():
    """the bf16 values in [0.5, 8) whose silu is further than SILU_MIN_MARGIN_FP32_ULP from a bf16 midpoint (exact_operands' SwiGLU margin), and whose
    fp32 and float64 silu round to the same word"""
    v = torch.arange(0x3F00, 0x4100, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).double()       # 0.5 .. 8 (exclusive)
    keep = silu_margins(v) >= SILU_MIN_MARGIN_FP32_ULP
    s64 = (v / (1 + torch.exp(-v))).to(torch.bfloat16)
    keep &= torch.nn.functional.silu(v.float()).to(torch.bfloat16) == s64
    return v[keep]


def draw_silu_inputs(M, K, seed, grid=None):
    """bf16 [M, K] from silu_safe_values(); grid: only multiples of it (for the a + a2 cases)"""
    vals = silu_safe_values()
    if grid:
        vals = vals[(vals / grid) == (vals / grid).round()]
    g = torch.Generator().manual_seed(seed)
    return vals[torch.randint(0, len(vals), (M, K), generator=g)].to(torch.bfloat16)


def split_sum(s, seed, grid=2.0 ** -4):
    """(a, a2) bf16 multiples of grid with a + a2 = s exactly (s: multiples of grid, >= 2 grid)"""
    g = torch.Generator().manual_seed(seed)
    n = (s.double() / grid).round()
    a = (torch.rand(s.shape, generator=g).double() * (n - 1)).floor() + 1
    a2 = n - a
    a, a2 = (a * grid).to(torch.bfloat16), (a2 * grid).to(torch.bfloat16)
    if not torch.equal(a.double() + a2.double(), s.double()):
        raise PreconditionError("a + a2 does not reproduce the drawn sum in bf16")
    return a, a2


def activated(a, a2=None, act_in=0):
    """the words the GEMV multiplies: R(a + a2) (a draw with an ambiguous sum is refused), then R(silu(.)) of silu-safe values -> float64 [M, K]"""
    x = d64(a)
    if a2 is not None:
        ch = Chain(x.shape).round(lambda _: x + d64(a2), sum2=True)
        if bool(ch.amb.any()):
            raise PreconditionError("a + a2: a sum lies within one fp32 rounding of a bf16 midpoint")
        x = ch.cands[0]
    if act_in == 1:
        safe = silu_safe_values()
        if not bool(torch.isin(x, safe).all()):
            raise PreconditionError("SiLU input outside the set whose rounded silu is unambiguous")
        x = rn(x / (1 + torch.exp(-x)))
    return x


def prep_mod_modes(N, L, chunks, d, final, tanh_mask, scale_mask, fault=None):
    """launch_prep_mod's transform per output column: 0 none, 1 tanh, 2 one-plus (column n in chunk (n / d) % chunks of a layer; past the layers the
    final layer's chunk `final` -> one-plus)"""
    n = np.arange(N)
    layers = L * chunks * d
    chn = (n // d) % chunks
    mode = np.where((tanh_mask >> chn) & 1, 1, np.where((scale_mask >> chn) & 1, 2, 0))
    if fault == "one_plus_as_tanh":
        mode = np.where(mode == 2, 1, mode)
    fin = (n >= layers + final * d) & (n < layers + (final + 1) * d) if final >= 0 else np.zeros(N, dtype=bool)
    return np.where(n < layers, mode, np.where(fin, 2, 0))


def ref_linear_small_m(x_act, W, bias, pm=None, fault=None):
    """x_act: the activated input words float64 [M, K] (activated()).  y = R(x W^T + b), then prep_mod's chain on the rounded word:
    R(tanh(y)) (DELTA_TANH) or R(1 + y).  pm: (L, chunks, d, final, tanh_mask, scale_mask) or None.  -> Chain over [M, N]"""
    y = rn(exact_linear(x_act, W, bias))
    ch = Chain(y.shape)
    if pm is None:
        ch.cands, ch.first = [y], y
        return ch
    mode = torch.from_numpy(prep_mod_modes(y.shape[1], *pm, fault=fault))[None, :].expand_as(y)
    th = Chain(y.shape).round(lambda _: torch.tanh(y), rel=DELTA_TANH)
    one = Chain(y.shape).round(lambda _: 1.0 + y, sum2=True)
    n = max(len(th.cands), len(one.cands))
    pick = lambda c, i: c.cands[min(i, len(c.cands) - 1)]
    ch.cands = [torch.where(mode == 1, pick(th, i), torch.where(mode == 2, pick(one, i), y)) for i in range(n)]
    ch.first = torch.where(mode == 1, th.first, torch.where(mode == 2, one.first, y))
    ch.amb = ((mode == 1) & th.amb) | ((mode == 2) & one.amb)
    return ch


def pick_timesteps(dim, count, seed=0):
    """timesteps in [0, 1] from a seeded list (0, 1 and 2^-10 first) for which NO feature word is ambiguous -> float32 tensor [count]"""
    g = torch.Generator().manual_seed(seed)
    cand = torch.cat([torch.tensor([0.0, 1.0, 2.0 ** -10]), torch.rand(64 * count, generator=g)]).float()
    amb = chain_timestep_features(cand, dim).amb.any(1)
    good = cand[~amb]
    if len(good) < count:
        raise PreconditionError(f"only {len(good)} of {len(cand)} candidate timesteps have unambiguous features at dim {dim}")
    return good[:count].contiguous()


# ---- comparators ----------------------------------------------------------------------------------------------------------------------------
def assert_words(got, ch, what):
    """got: bf16 tensor of the chain's shape -> ambiguous share (exact_rows.assert_row_words: cap, candidates, located failures)"""
    return R.assert_row_words(got.detach().cpu().reshape(ch.amb.shape), ch, what)


def assert_f32_holds_bf16(got, ch, what):
    """an fp32 output that must hold a bf16-valued word: the value survives bf16, then the word comparison"""
    g = got.detach().cpu().float().reshape(ch.amb.shape)
    lost = g.to(torch.bfloat16).float() != g
    lost &= ~torch.isnan(g)
    assert not bool(lost.any()), f"{what}: {int(lost.sum())} fp32 words are not bf16 values; first at {lost.nonzero()[:3].tolist()}"
    return R.assert_row_words(g.to(torch.bfloat16), ch, what)


def assert_within(got, val, err, what):
    """fp32 words against float64 values with a per-word absolute bound -> the largest |got - val| / bound.  Locates the first wrong words"""
    g = got.detach().cpu().double().reshape(val.shape)
    dist = (g - val).abs()
    bad = ~(dist <= err)
    if bool(bad.any()):
        idx = bad.nonzero()
        first = [(i, float(g[tuple(i)]), float(val[tuple(i)]), float(err[tuple(i)])) for i in idx[:4].tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} words outside the bound; index range {idx.min(0)[0].tolist()}..{idx.max(0)[0].tolist()}; "
                             f"first (index, got, float64, bound): {first}")
    return float((dist / err.clamp_min(1e-300)).max())


def worst_distance(got, ch):
    """largest distance of a written word from the float64 pre-image, in units of half its bf16 spacing (1.0 = a word at the edge of RN's interval)"""
    g = got.detach().cpu().double().reshape(ch.first.shape)
    _, lo, hi, _ = neighbours(ch.first, 0.0)
    half = ((hi.double() - lo.double()).abs() / 2).clamp_min(1e-300)
    ok = torch.isfinite(g) & (ch.first != 0)
    return float(((g - ch.first).abs() / half)[ok].max()) if bool(ok.any()) else 0.0


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
