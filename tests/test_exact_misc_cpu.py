"""CPU: the references and comparators of tests/exact_misc.py against fp32 restatements of the same chains (torch / numpy float32, the reference's own
tensor expressions where there is one): zero wrong words, every case of the GPU table under the ambiguity cap on the reference alone, the measured
fp32-against-float64 errors below the derived bounds; and a list of planted local faults, each of which must be caught AND located - one of them is
shown to pass a 2.5e-2 rel-L2 gate on the same data."""
import math

import numpy as np
import pytest
import torch

import exact_misc as M
import exact_rows as R
import test_gpu_misc_exact as G
from exact_operands import PreconditionError, int_bias

r16 = lambda t: t.to(torch.bfloat16).float()


def _caught(fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    assert "wrong" in msg or "outside" in msg, msg
    for n in needles:
        assert n in msg, (n, msg)
    return msg


# ---- conversions and movement -----------------------------------------------------------------------------------------------------------------
def test_integer_rounding_agrees_with_torch_and_truncation_is_caught():
    x = M.special_f32(5000, 1)
    want, nan = M.convert_words(x)                       # (cross-checks torch's cast itself)
    assert int(nan.sum()) >= 4 and bool(np.isinf(x.numpy()).any())
    u = x.view(torch.int32).numpy().view(np.uint32)
    ties = (u & 0xFFFF) == 0x8000
    assert int((ties & ((u >> 16) & 1 == 0)).sum()) > 0 and int((ties & ((u >> 16) & 1 == 1)).sum()) > 0, "ties of both parities"
    up_to_inf = (u & 0x7FFFFFFF) == 0x7F7FFFFF
    assert bool(((want[up_to_inf].astype(np.int64) & 0x7FFF) == 0x7F80).all()), "the largest finite values round to inf"
    h = M.special_f16(5000, 2)
    w16, n16 = M.convert_words(h)
    assert int(n16.sum()) > 0
    trunc, _ = M.convert_words(x, fault="truncate")
    msg = _caught(lambda: M.assert_bits(trunc, want, "cast", nan))
    assert "first (index, got, want)" in msg
    M.assert_bits(want, want, "cast", nan)


@pytest.mark.parametrize("c", G.PATCHIFY[:9], ids=str)
def test_patchify_reference_is_the_tensor_expression(c):
    xd, B, Cc, H, W, p, kpad, dup, eol = c
    Hp, Wp = H // p, W // p
    x = M.random_words((B, Cc, H, W), 3)
    src = torch.cat([x[:B // 2], x[:B // 2]]) if dup else x
    rows = src.view(torch.int16).view(B, Cc, Hp, p, Wp, p).permute(0, 2, 4, 1, 3, 5).flatten(3)      # model.py:776-777
    wps = Wp + 1 if eol else 0
    want = M.ref_patchify(M.bits(x), p, kpad, dup, wps).reshape(B, Hp, Wp + eol, kpad)
    assert np.array_equal(want[:, :, :Wp, :Cc * p * p], rows.numpy()) and bool((want[:, :, :Wp, Cc * p * p:] == 0).all())
    if eol:
        assert bool((want[:, :, Wp] == M.SENT16).all())
        bad = M.ref_patchify(M.bits(x), p, kpad, dup, wps, fault="eol_not_skipped")
        _caught(lambda: M.assert_bits(bad, want.reshape(bad.shape), "patchify"), "sentinel")


def test_upload_row_map_without_its_offset_is_caught():
    src = M.random_words((96 * 24,), 5)
    w, _ = M.convert_words(src)
    want, nm = M.ref_upload_rows(w, None, 96, 24, 40, 0, 2, 194)
    bad, _ = M.ref_upload_rows(w, None, 96, 24, 40, 0, 2, 194, fault="no_plus_32")
    msg = _caught(lambda: M.assert_bits(bad, want, "upload_rows row_map 2"))
    assert "[0, 0]" in msg                                # the first wrong row is row 0 (it should have stayed untouched)
    assert bool((want[:32] == M.SENT16).all()) and bool((want[32:64, 24:] == M.SENT16).all())
    one, _ = M.ref_upload_rows(w, None, 96, 24, 40, 0, 1, 194)
    assert np.array_equal(one[:32, :24], want[32:64, :24])


# ---- chains: the fp32 machine's words pass, planted faults do not -----------------------------------------------------------------------------
def emu_cfg(rows, B, Cc, och, H, W, p, use_cfg, s, cfgc, wps):
    x = M.unpatchify_index(rows.float(), B, Cc, och, H, W, p, wps)
    if use_cfg:
        half = B // 2
        cond, unc = x[:half, :cfgc], x[half:, :cfgc]
        st = torch.tensor(s, dtype=torch.float32)
        v = r16(unc + r16(st * r16(cond - unc)))
        x = x.clone()
        x[:half, :cfgc], x[half:, :cfgc] = v, v
    return x.reshape(B * Cc, H * W).to(torch.bfloat16)


@pytest.mark.parametrize("c", G.UNPATCH[:8], ids=str)
def test_cfg_chain_and_its_faults(c):
    od, B, Cc, och, H, W, p, extra, use_cfg, s, cfgc, eol = c
    Hp, Wp = H // p, W // p
    wps = Wp + 1 if eol else 0
    rows = R.draw_rows(B * Hp * (Wp + eol), p * p * och + extra, sum(map(int, c[:9])), std=1.0)
    args = (rows, B, Cc, och, H, W, p, use_cfg, s, cfgc, wps)
    ch = M.ref_unpatchify_cfg(*args)
    got = emu_cfg(*args)
    M.assert_words(got, ch, "cfg")
    M.assert_f32_holds_bf16(got.float(), ch, "cfg fp32")
    # (at s = 4.0 the product is an exact scaling: R(4 R(x)) = R(4 x), the inner rounding cannot be missed - the fault exists at s = 4.3 only)
    faults = (["swap_cond_uncond"] if use_cfg else []) + (["no_inner_round"] if use_cfg and s != 4.0 else []) + (["eol_not_skipped"] if eol else [])
    for f in faults:
        bad = M.ref_unpatchify_cfg(*args, fault=f).want.to(torch.bfloat16)
        msg = _caught(lambda: M.assert_words(bad, ch, f), "first: (row")
        if f == "no_inner_round":                         # a word moves by one bf16 ulp: the model-level gate does not see it
            rel = M.rel_l2(bad, got)
            assert 0 < rel < 2.5e-2, rel
            print(f"CFG chain without its inner rounding: rel-L2 {rel:.3e} against the correct words - passes a 2.5e-2 gate; {msg[:80]}")


@pytest.mark.parametrize("c", G.REGION[:7], ids=str)
def test_region_chain_and_its_faults(c):
    Y, Hp, Wp, hs, ws = c
    H, hd = 2, 72
    N, d = Hp * Wp, H * hd
    out0, txt = R.draw_rows(2 * N, d, sum(c), std=1.0), R.draw_rows(Y * N, d, sum(c) + 1, std=1.0)
    for gate in ([20.0, -20.0], [0.0, 0.37], [2.0 ** -9, -1.5]):
        gt = torch.tensor(gate).to(torch.bfloat16)
        ch = M.ref_region_text_combine(out0, txt, gt, Y, N, H, hd, Hp, Wp, hs, ws)
        reg = torch.from_numpy(M.region_index(N, Hp, Wp, hs, ws))
        use = (reg >= 0) & (reg < Y - 1)
        t = txt.float().view(Y, N, d)
        sel = torch.where(use[:, None], t[reg.clamp(0, Y - 1), torch.arange(N)], torch.zeros(N, d))
        g = r16(torch.tanh(gt.float())).repeat_interleave(hd)[None, :]
        got = (out0.float() + r16(torch.cat([sel, t[Y - 1]]) * g)).to(torch.bfloat16)
        M.assert_words(got, ch, f"region {c} {gate}")
    if hs * ws > 1 and Y > 2:
        bad = M.ref_region_text_combine(out0, txt, gt, Y, N, H, hd, Hp, Wp, hs, ws, fault="no_minus_1").want.to(torch.bfloat16)
        _caught(lambda: M.assert_words(bad, ch, "region"), "(row 0, col")     # token 0 lies in cell (0, 0): caption 0, not 1


def test_region_index_is_the_reference_mask():
    """model.py:872-887 executed literally: one mask per caption; a token has at most one regional caption"""
    for Y, Hp, Wp, hs, ws in G.REGION[:7]:
        mask = torch.zeros(max(Y, hs * ws + 1), Hp, Wp)
        hp, wp = Hp // hs, Wp // ws
        for i in range(hs):
            for j in range(ws):
                mask[(i + 1) * (j + 1) - 1, hp * i:hp * (i + 1), wp * j:wp * (j + 1)] = 1
        regional = mask[:-1] if mask.shape[0] == Y else mask[:hs * ws]
        assert int(regional.sum(0).max()) <= 1
        reg = M.region_index(Hp * Wp, Hp, Wp, hs, ws)
        for r in range(regional.shape[0]):
            assert np.array_equal(regional[r].reshape(-1).numpy() > 0.5, reg == r)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_ode_chains_are_torch_arithmetic_and_a_contraction_is_caught(mode):
    for n in (1, 255, 256, 257, 5000):
        for dt in (0.125, -0.0390625, 0.3, -0.0123):
            g = torch.Generator().manual_seed(mode * 7 + n)
            ts = [torch.randn(n, generator=g) * s for s in (1.0, 0.7, 0.8, 0.9, 0.6)]

            def torch_expr(y0, k1, k2, k3, k4, dt_):     # torchdiffeq: fixed_grid.py (euler / midpoint), rk_common.rk4_alt_step_func
                third = 1 / 3
                return [lambda: y0 + dt_ * k1, lambda: y0 + dt_ * k1 * third, lambda: y0 + dt_ * (k2 - k1 * third), lambda: y0 + dt_ * (k1 - k2 + k3),
                        lambda: y0 + (k1 + 3 * (k2 + k3) + k4) * dt_ * 0.125][mode]()
            want = M.ref_ode_combine_f32(mode, *ts, dt)
            got = torch_expr(*ts, torch.tensor(dt, dtype=torch.float32))
            M.assert_bits(M.bits(got), want.view(np.int32), f"fp32 ode mode {mode}")
            tb = [t.to(torch.bfloat16) for t in ts]
            dtb = torch.tensor(dt).to(torch.bfloat16)
            ch = M.ref_ode_combine_bf16(mode, *tb, float(dtb))
            M.assert_words(torch_expr(*tb, dtb), ch, f"bf16 ode mode {mode} n {n} dt {dt}")
    if mode in (2, 4):
        fused = M.ref_ode_combine_f32(mode, *ts, dt, fault="fma")
        msg = _caught(lambda: M.assert_bits(fused.view(np.int32), want.view(np.int32), "fp32 ode"), "first (index, got, want)")
        nbad = int((fused != want).sum())
        assert 0 < nbad < want.size and M.rel_l2(torch.from_numpy(fused), torch.from_numpy(want)) < 1e-6, (nbad, msg)


def torch_timestep_embedding(t, dim, max_period=10000):
    """model.py:63-82"""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


@pytest.mark.parametrize("dim", [256, 32, 34])
def test_timestep_bound_admits_the_reference_expression_and_catches_faults(dim):
    g = torch.Generator().manual_seed(dim)
    t = torch.cat([torch.tensor([0.0, 1.0, 2.0 ** -10]), torch.rand(253, generator=g)])
    val, err = M.ref_timestep_features(t, dim)
    emb = torch_timestep_embedding(t, dim)
    worst = float(((emb.double() - val).abs() / err.clamp_min(1e-300)).max())
    print(f"timestep dim {dim}: fp32 torch expression at most {worst:.3f} of the bound (margin {M.MARGIN})")
    assert worst * M.MARGIN < 1.0, "the measured fp32 error must stay below the derived (unmargined) bound"
    ch = M.chain_timestep_features(t, dim)
    share = M.assert_words(emb.to(torch.bfloat16), ch, "timestep")
    assert share < M.MAX_AMBIGUOUS
    for f, where in (("swap_cos_sin_at_k1", "(row 0, col 1:"), ("half_minus_1", "(row 1, col")):       # (row 0 is t = 0: every frequency gives cos 1, sin 0)
        bad = M.ref_timestep_features(t, dim, fault=f)[0].to(torch.bfloat16)
        msg = _caught(lambda: M.assert_words(bad, ch, f), where)
        if f == "half_minus_1" and dim == 256:
            rel = M.rel_l2(bad, emb)
            print(f"k / (half - 1): rel-L2 {rel:.3e}")
    assert len(M.pick_timesteps(dim, 8, 3)) == 8


@pytest.mark.parametrize("c", G.ROPE, ids=str)
def test_rope_bound_admits_the_reference_expression(c):
    ln, hd, step, th0, l0, th1, l1, lop, with_t = c
    val, err = M.ref_rope_table(ln, hd, step, th0, l0, th1, l1, lop)
    outs = []
    for th, lin in ((th0, l0), (th1, l1)):               # precompute_freqs_cis, fp32 tensors
        freqs = 1.0 / (th ** (torch.arange(0, hd, step)[: hd // step].float() / hd))
        pos = torch.arange(ln, dtype=torch.float32)
        ang = torch.outer(pos / lin, freqs) if lop else torch.outer(pos, freqs / lin)
        outs.append(torch.stack([torch.cos(ang), torch.sin(ang)], -1))
    got = torch.stack(outs)
    worst = M.assert_within(got, val, err, f"rope {c}")
    print(f"rope {c}: fp32 torch expression at most {worst:.3f} of the bound")
    assert worst * M.MARGIN < 1.0
    tr = got.permute(0, 2, 1, 3).contiguous()
    if ln > 1:
        _caught(lambda: M.assert_bits(M.bits(got.reshape(tr.shape)), M.bits(tr), "out_t"), "first (index, got, want)")
    shifted = got.clone()
    shifted[1, ln - 1, 0, 1] += 4 * float(err[1, ln - 1, 0, 1]) + 1e-6
    _caught(lambda: M.assert_within(shifted, val, err, "rope"), "outside the bound")


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("Cc", [64, 300, 2048])
@pytest.mark.parametrize("T", [1, 16, 77])
def test_cap_pool_ln_chain_and_its_faults(T, Cc, bf16):
    cap, mask = G._caption(3, T, Cc, T + Cc, bf16)
    w, bb = R.draw_vec(Cc, Cc + 1, 1.0), R.draw_vec(Cc, Cc + 2, 0.0)
    ch = M.ref_cap_pool_ln(cap, mask, w, bb, bf16)
    m = mask.float()
    pooled = ((cap.float() * m[:, :, None]).sum(1) / m.sum(1, keepdim=True)).to(cap.dtype)        # model.py:847-849
    assert torch.equal(pooled.double(), M.pooled_caption(cap, mask, bf16))
    for order in ("kernel", "torch"):
        x = pooled.float()
        if order == "torch":
            got = torch.nn.functional.layer_norm(x, (Cc,), w.float(), bb.float(), 1e-5)
        else:                                              # serial per thread, the wave butterfly, then four partials
            def red(v):
                pad = torch.zeros(v.shape[0], (Cc + 255) // 256 * 256)
                pad[:, :Cc] = v
                lanes = torch.zeros(v.shape[0], 256)
                for i in range(pad.shape[1] // 256):
                    lanes = lanes + pad[:, 256 * i:256 * (i + 1)]
                q = R._butterfly(lanes.view(v.shape[0], 4, 64))
                return ((q[:, 0] + q[:, 1] + q[:, 2] + q[:, 3]) / float(Cc))[:, None]
            mean = red(x)
            rstd = torch.rsqrt(red((x - mean) * (x - mean)) + torch.tensor(1e-5))
            got = (x - mean) * rstd * w.float() + bb.float()
        share = M.assert_words(got.to(torch.bfloat16), ch, f"cap_pool_ln {order}")
    x64 = pooled.double()
    mean64, rstd64, mabs = R.ln_stats(x64, 1e-5)
    cm, cr = M.cap_ln_derived(Cc)
    assert bool(((mean.double() - mean64).abs() <= cm * mabs).all()) and bool(((rstd.double() - rstd64).abs() <= cr * rstd64).all()), "measured statistic error above the derived bound"
    if T > 1:
        bad = M.ref_cap_pool_ln(cap, mask, w, bb, bf16, fault="mean_over_T").want.to(torch.bfloat16)
        _caught(lambda: M.assert_words(bad, ch, "cap_pool_ln"), "row {")


@pytest.mark.parametrize("c", G.ROUTE, ids=str)
def test_router_reference_accepts_fp32_routing(c):
    E, d, rows, forced, tie = c
    rows = min(rows, 300)
    x = R.draw_rows(rows, d, sum(c), std=1.0)
    rw = R.draw_vec(E * d, d + E, 0.0, 0.05).view(E, d).clone()
    if tie:
        rw[E - 1] = rw[1]
    logit = r16(x.float() @ rw.float().t())
    sel, wts = [], []
    for r in range(rows):
        i1, i2 = R._top2(logit[r].tolist())
        ex = math.exp(float(logit[r, i2] - logit[r, i1]))
        wa, wb = 1 / (1 + ex), ex / (1 + ex)
        if i2 < i1:
            i1, i2, wa, wb = i2, i1, wb, wa
        sel.append([i1, i2])
        wts.append([wa, wb])
    sel, wts = torch.tensor(sel, dtype=torch.int32), torch.tensor(wts).to(torch.bfloat16)
    R.check_routing(x, rw, sel, wts, None, "route")
    if tie:
        assert not bool((sel == E - 1).any(1).logical_and(~(sel == 1).any(1)).any())
        bad = sel.clone()
        hit = (sel[:, 0] == 1).nonzero()
        if len(hit):
            bad[hit[0, 0], 0], bad[hit[0, 0], 1] = sorted([E - 1, int(sel[hit[0, 0], 1])]) if int(sel[hit[0, 0], 1]) != E - 1 else (1, E - 1)
            if not torch.equal(bad, sel):
                _caught(lambda: R.check_routing(x, rw, bad, wts, None, "route"), "routing wrong")


# ---- linear_small_m: every case of the GPU table on the reference alone -----------------------------------------------------------------------
def test_silu_safe_set_is_large_and_margined():
    v = M.silu_safe_values()
    assert len(v) > 400 and float(v.min()) >= 0.5 and float(v.max()) < 8.0


@pytest.mark.parametrize("K", G.ALL_K)
@pytest.mark.parametrize("N", G.ALL_N)
def test_linear_cases_meet_the_exactness_precondition(N, K):
    for Mr in G.ALL_M:
        seed = Mr * 1000 + N + K
        a, w = M.draw_silu_inputs(Mr, K, seed), M.pow2_weights(N, K, seed + 1)
        bias = int_bias(N, torch.Generator().manual_seed(seed)).to(torch.bfloat16) if (Mr + N + K) % 2 else None
        ch = M.ref_linear_small_m(M.activated(a, None, 1), w, bias)
        x = r16(torch.nn.functional.silu(a.float()))
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(1))
        y = (x[:, perm] @ w.float()[:, perm].t() + (bias.float() if bias is not None else 0.0)).to(torch.bfloat16)      # another summation order
        M.assert_words(y, ch, f"linear M {Mr} N {N} K {K}")


@pytest.mark.parametrize("extras", ["a2", "a2+silu", "pm", "a2+silu+pm", "t", "t+a2+pm"])
def test_linear_extras_on_the_reference_alone_and_the_prep_mod_fault(extras):
    use = set(extras.split("+"))
    for Mr in G.ALL_M:
        K = 256 if "t" in use else 560
        N = 2 * K + 5 if "t" in use else G.PM_N
        seed = Mr * 31 + len(extras)
        act = 1 if "silu" in use else 0
        a2 = None
        if "t" in use:
            t = M.pick_timesteps(K, Mr, seed)
            x32 = r16(torch_timestep_embedding(t, K))
            assert torch.equal(x32.double(), M.chain_timestep_features(t, K).want), "unambiguous features are the reference's words"
            w = M.selector_weights(N, K, seed + 1)
            if "a2" in use:
                a2 = (torch.randint(-8, 9, (Mr, K), generator=torch.Generator().manual_seed(seed)).float() / 4).to(torch.bfloat16)
                x32 = r16(x32 + a2.float())
            x = M.activated(x32.to(torch.bfloat16), None, 0)
            assert int((w != 0).sum()) == N and bool(((w != 0).sum(0) >= 2).all())
        else:
            s = M.draw_silu_inputs(Mr, K, seed, grid=2.0 ** -4)
            a, a2 = M.split_sum(s, seed + 2) if "a2" in use else (s, None)
            x = M.activated(a, a2, act)
            x32 = a.float() if a2 is None else r16(a.float() + a2.float())
            x32 = r16(torch.nn.functional.silu(x32)) if act else x32
            w = M.pow2_weights(N, K, seed + 1)
        pm = G.PM if "pm" in use else None
        ch = M.ref_linear_small_m(x, w, None, pm)
        y = r16(x32 @ w.float().t())
        if pm:
            mode = torch.from_numpy(M.prep_mod_modes(N, *pm))[None, :]
            y = torch.where(mode == 1, r16(torch.tanh(y)), torch.where(mode == 2, r16(1.0 + y), y))
            assert set(np.unique(M.prep_mod_modes(N, *pm)[104:125]).tolist()) == {0, 2} and len(set(M.prep_mod_modes(N, *pm)[8:16].tolist())) == 2
        M.assert_words(y.to(torch.bfloat16), ch, f"linear ext {extras} M {Mr}")
        if pm:
            bad = M.ref_linear_small_m(x, w, None, pm, fault="one_plus_as_tanh").want.to(torch.bfloat16)
            _caught(lambda: M.assert_words(bad, ch, "prep_mod"), "first: (row")


def test_add_chain_and_ambiguous_sums_are_refused():
    a, b = G._vals(5000, 1), G._vals(5000, 2, 0.3)
    M.assert_words((a.float() + b.float()).to(torch.bfloat16), M.chain_add(a, b), "add")
    x = torch.tensor([[1.0]], dtype=torch.bfloat16)
    with pytest.raises(PreconditionError):
        M.activated(x, torch.tensor([[2.0 ** -8 + 2.0 ** -30]]).to(torch.float32), 0)
