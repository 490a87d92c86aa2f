"""CPU: rescaled and norm-limited guidance - transport/guidance.py: guided_rule / sample_cfg_rule.  No GPU.

* ``guided_rule`` against a restatement written out element by element: numpy fp32 / float64 scalars and an explicit bf16 rounding helper;
* rule off (``rescale = 0``, ``norm_limit = inf``): ``f == 1.0`` exactly, and ``sample_cfg_rule`` around a torch toy model IS ``sample_cfg_schedule``;
* the norm limit engages for some samples only and holds up to the last rounding; ``rescale = 1`` restores the conditional output's std;
* degenerate inputs never give NaN; bad parameters are refused; the ``sample.py`` defaults build no rule.

The bounds: step 4 rounds ``g * f`` to bf16 once per element - relative 2^-8 per element (bf16 keeps 8 significand bits; half an ulp is 2^-9) -
on top of the fp32 product and the fp32 rounding of ``f`` (2^-24 each) and the float64 factor arithmetic (a few 2^-53): ``(1 + 2^-8)(1 + 2^-20)``
on a norm; the std of a zero-mean sample moves by at most the rms of the element errors, the same relative 2^-8."""
import math

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE

STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
NORM_BOUND = (1.0 + 2.0 ** -8) * (1.0 + 2.0 ** -20)
STD_BOUND = 2.0 ** -8


def bf16_round(x):
    """an fp32 value rounded to the nearest bf16 (ties to even), as an np.float32"""
    u = int(np.float32(x).view(np.uint32))
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return np.uint32(u).view(np.float32)


def restated(o, w, ch, rescale, norm_limit):
    """guided_rule element by element: (out [B, C, H, W] fp32 array of bf16 values, f [B / 2] fp32)"""
    o = o.float().numpy()
    B, C, H, W = o.shape
    half = B // 2
    rescale, norm_limit = float(np.float32(rescale)), float(np.float32(norm_limit))
    w32 = np.float32(w)
    out = o.copy()
    fs = np.zeros(half, dtype=np.float32)
    n = float(ch * H * W)
    for b in range(half):
        g = np.zeros((ch, H, W), dtype=np.float32)
        terms = [[], [], [], []]
        for c in range(ch):
            for i in range(H):
                for j in range(W):
                    cond, unc = o[b, c, i, j], o[b + half, c, i, j]
                    g[c, i, j] = bf16_round(unc + bf16_round(w32 * bf16_round(cond - unc)))
                    dc, dg = float(cond), float(g[c, i, j])
                    for lst, v in zip(terms, (dc, dc * dc, dg, dg * dg)):
                        lst.append(v)
        Sc, Scc, Sg, Sgg = (math.fsum(t) for t in terms)
        mc, mg = Sc / n, Sg / n
        vc, vg = Scc / n - mc * mc, Sgg / n - mg * mg
        ratio = math.sqrt(vc / vg) if (vg > 0.0 and vc >= 0.0) else 1.0
        fr = rescale * ratio + (1.0 - rescale)
        fl = 1.0
        if norm_limit < math.inf and fr * math.sqrt(Sgg) > 0.0:
            fl = min(1.0, norm_limit * math.sqrt(Scc) / (fr * math.sqrt(Sgg)))
        fs[b] = np.float32(fr * fl)
        for c in range(ch):
            for i in range(H):
                for j in range(W):
                    v = bf16_round(g[c, i, j] * fs[b])
                    out[b, c, i, j] = v
                    out[b + half, c, i, j] = v
    return out, fs


def _amplitude_rows(B, C, H, W, seed, amps=(0.25, 1.0, 4.0)):
    """cond rows of unit scale, uncond row b scaled by amps[b]: |g| / |c| spans a norm limit between the samples"""
    g = torch.Generator().manual_seed(seed)
    half = B // 2
    cond = torch.randn(half, C, H, W, generator=g)
    unc = torch.randn(half, C, H, W, generator=g) * torch.tensor([amps[b % len(amps)] for b in range(half)]).view(-1, 1, 1, 1)
    return torch.cat([cond, unc]).to(torch.bfloat16)


@pytest.mark.parametrize("ch", [3, 4])
def test_guided_rule_equals_the_element_by_element_restatement(ch):
    o = _amplitude_rows(4, 4, 6, 10, seed=20 + ch)
    for w, rescale, limit in ((4.0, 0.0, math.inf), (4.0, 0.7, math.inf), (7.5, 0.0, 1.5), (7.5, 1.0, 1.5), (-1.5, 0.3, 0.75), (0.0, 0.7, 2.0)):
        got, f = G.guided_rule(o, w, ch, rescale, limit)
        want, fw = restated(o, w, ch, rescale, limit)
        assert got.dtype == torch.bfloat16 and got.shape == o.shape and f.dtype == torch.float32 and f.shape == (2,)
        assert np.array_equal(f.numpy().view(np.uint32), fw.view(np.uint32)), (w, rescale, limit, f, fw)
        assert np.array_equal(got.float().numpy().view(np.uint32), want.view(np.uint32)), (w, rescale, limit)
        assert torch.equal(got[:, ch:], o[:, ch:])  # the channels past ch pass through, row by row
        # an fp32 tensor of the same values (what an engine-backed model hands an fp32 state) gives the same words in fp32
        got32, f32 = G.guided_rule(o.float(), w, ch, rescale, limit)
        assert got32.dtype == torch.float32 and torch.equal(got32, got.float()) and torch.equal(f32, f)


class Toy:
    """a torch 'model' with a bf16 output: forward, and the reference's forward_with_cfg (guidance on the first cfg_channels channels)"""
    cfg_channels = 3

    def net(self, x, t, y):
        xb = x.to(torch.bfloat16)
        return torch.tanh(xb * y.view(-1, 1, 1, 1).to(xb.dtype)) - t.view(-1, 1, 1, 1).to(xb.dtype) * xb

    def forward(self, x, t, y):
        assert t.dtype == torch.float32 and t.shape[0] == x.shape[0] == y.shape[0]
        return self.net(x, t, y).to(x.dtype)

    def forward_with_cfg(self, x, t, y, cfg_scale):
        half = x[: len(x) // 2]
        out = self.net(torch.cat([half, half]), t, y)
        eps, rest = out[:, :3], out[:, 3:]
        cond, unc = eps.chunk(2)
        g = unc + cfg_scale * (cond - unc)
        return torch.cat([torch.cat([g, g]), rest], dim=1).to(x.dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_rule_off_is_factor_one_and_the_schedule_loop_bit_for_bit(method, dtype):
    o = _amplitude_rows(4, 4, 6, 10, seed=5)
    for w in (0.0, 4.0, 7.5, -1.5):
        got, f = G.guided_rule(o, w, 3)
        assert f.tolist() == [1.0, 1.0]
        c, u = o[:2, :3], o[2:, :3]
        g = u + w * (c - u)
        assert torch.equal(got, torch.cat([torch.cat([g, o[:2, 3:]], 1), torch.cat([g, o[2:, 3:]], 1)]))
    tgrid = ODE(6, method, 4.0).t
    n = (len(tgrid) - 1) * STAGES[method]
    z = torch.randn(2, 4, 4, 6, generator=torch.Generator().manual_seed(2)).to(dtype).repeat(2, 1, 1, 1)
    y = torch.tensor([0.5, -1.25, 2.0, 0.75])
    table = torch.tensor([1.0 if i % 3 == 1 else 1.5 + i for i in range(n)])
    toy = Toy()
    want = G.sample_cfg_schedule(toy, z, tgrid, table, method, y=y)
    factors = []
    got = G.sample_cfg_rule(toy, z, tgrid, table, method, y=y, factors=factors)
    assert got.dtype == dtype and torch.equal(got, want) and bool(torch.isfinite(got.float()).all())
    assert len(factors) == int((table != 1).sum()) and all(f.tolist() == [1.0, 1.0] for f in factors)
    # with the rule on the trajectory moves; the front end makes the same two calls for a CPU state
    on = G.sample_cfg_rule(toy, z, tgrid, table, method, rescale=0.7, norm_limit=1.0, y=y)
    assert bool(torch.isfinite(on.float()).all()) and not torch.equal(on[-1], want[-1])
    o_ = ODE(6, method, 4.0)
    assert torch.equal(o_.sample(z, toy.forward_with_cfg, cfg_table=table, y=y, cfg_scale=9.0), want)
    assert torch.equal(o_.sample(z, toy.forward_with_cfg, cfg_table=table, cfg_rescale=0.7, cfg_norm_limit=1.0, y=y, cfg_scale=9.0), on)
    # without a table: cfg_scale at every stage
    const = G.sample_cfg_rule(toy, z, tgrid, torch.full((n,), 3.0), method, rescale=0.7, y=y)
    assert torch.equal(o_.sample(z, toy.forward_with_cfg, cfg_rescale=0.7, y=y, cfg_scale=3.0), const)


def _norms(t):
    return t.double().reshape(t.shape[0], -1).norm(dim=1)


def r_mid(o, w, ch, rescale):
    """a limit between the smallest and the largest fr |g| / |c| of the samples, from the reference's own factors: an fp32 value"""
    parts = []
    G.guided_rule(o, w, ch, rescale, math.inf, parts)
    half = o.shape[0] // 2
    ob = o.to(torch.bfloat16)
    c, u = ob[:half, :ch], ob[half:, :ch]
    q = [fr * float(x) for (fr, _), x in zip(parts, _norms(u + w * (c - u)) / _norms(c))]
    assert min(q) * 1.05 < max(q), q
    return float(np.float32(math.sqrt(min(q) * max(q))))


@pytest.mark.parametrize("ch", [3, 4])
def test_norm_limit_engages_for_some_samples_and_holds_up_to_the_last_rounding(ch):
    o = _amplitude_rows(6, 4, 6, 10, seed=31)
    w = 4.0
    for rescale in (0.0, 0.5):
        r = r_mid(o, w, ch, rescale)
        parts = []
        got, f = G.guided_rule(o, w, ch, rescale, r, parts)
        fls = [fl for _, fl in parts]
        assert any(fl < 1.0 for fl in fls) and any(fl == 1.0 for fl in fls), fls
        nc, ngg = _norms(o[:3, :ch]), _norms(got[:3, :ch])
        print("norm ratios |gg| / (r |c|):", (ngg / (r * nc)).tolist(), "fl:", fls)
        assert bool((ngg <= r * nc * NORM_BOUND).all()), (ngg / (r * nc)).tolist()
        assert torch.equal(got[:3, :ch], got[3:, :ch])


@pytest.mark.parametrize("ch", [3, 4])
def test_full_rescale_restores_the_conditional_std(ch):
    o = _amplitude_rows(6, 4, 6, 10, seed=32)
    got, f = G.guided_rule(o, 7.5, ch, 1.0, math.inf)
    sc = o[:3, :ch].double().reshape(3, -1).std(dim=1, unbiased=False)
    sg = got[:3, :ch].double().reshape(3, -1).std(dim=1, unbiased=False)
    print("std ratios:", (sg / sc).tolist(), "f:", f.tolist())
    assert bool(((sg / sc - 1.0).abs() <= STD_BOUND).all()), (sg / sc).tolist()
    assert bool((f < 1.0).all())  # guidance at 7.5 widens the output: the factor shrinks it


def test_degenerate_inputs_give_one_or_a_finite_factor_never_nan():
    g = torch.Generator().manual_seed(4)
    c = torch.randn(2, 4, 6, 10, generator=g).to(torch.bfloat16)
    for rescale, limit in ((0.7, math.inf), (0.0, 1.0), (1.0, 2.0)):
        out, f = G.guided_rule(torch.cat([c, c]), 4.0, 3, rescale, limit)  # c == u: g is c
        assert f.tolist() == [1.0, 1.0] and torch.equal(out, torch.cat([c, c]))
        out, f = G.guided_rule(torch.cat([c, torch.zeros_like(c)]), 0.0, 3, rescale, limit)  # g == 0 everywhere
        assert f.tolist() == [1.0, 1.0] and bool((out[:, :3] == 0).all())
        out, f = G.guided_rule(torch.cat([c, torch.full_like(c, 0.5)]), 0.0, 3, rescale, limit)  # g constant: no variance to match
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(out.float()).all())
        if rescale == 0.7:
            assert f.tolist() == [1.0, 1.0]
        out, f = G.guided_rule(torch.cat([torch.zeros_like(c), c]), 4.0, 3, rescale, limit)  # c == 0: nothing to pull towards
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(out.float()).all())


def test_bad_parameters_are_refused_and_the_driver_defaults_build_no_rule():
    o = _amplitude_rows(4, 4, 2, 2, seed=1)
    for rescale in (1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rescale"):
            G.guided_rule(o, 4.0, 3, rescale, math.inf)
    for limit in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="norm_limit"):
            G.guided_rule(o, 4.0, 3, 0.0, limit)
    with pytest.raises(ValueError, match="even batch"):
        G.guided_rule(o[:3], 4.0, 3, 0.5, 1.0)
    toy, tgrid = Toy(), ODE(3, "euler").t
    z, y = torch.zeros(2, 4, 2, 2), torch.ones(2)
    with pytest.raises(ValueError, match="rescale"):
        G.sample_cfg_rule(toy, z, tgrid, [4.0, 4.0], "euler", rescale=2.0, y=y)
    with pytest.raises(ValueError, match="norm_limit"):
        ODE(3, "euler").sample(z, toy.forward_with_cfg, cfg_norm_limit=0.0, y=y, cfg_scale=4.0)
    assert G.rule_is_off(0.0, math.inf) and not G.rule_is_off(0.0, 1.0) and not G.rule_is_off(0.1, math.inf)

    from lumina_t2x_amd import sample as S
    args = S.build_parser().parse_args(["--ckpt", "nowhere"])
    assert args.cfg_rescale == 0.0 and args.cfg_norm_limit is None
    assert S.guidance_rule(args) == {} and S.guidance_table(args, ODE(5, "euler").t) is None  # run() then makes the plain sampler call
    args = S.build_parser().parse_args(["--ckpt", "nowhere", "--cfg_rescale", "0.5", "--cfg_norm_limit", "1.25", "--cfg_interval", "0.1", "0.8"])
    assert S.guidance_rule(args) == dict(cfg_rescale=0.5, cfg_norm_limit=1.25) and S.guidance_table(args, ODE(5, "euler").t) is not None
    with pytest.raises(ValueError, match="rescale"):
        S.guidance_rule(S.build_parser().parse_args(["--ckpt", "nowhere", "--cfg_rescale", "1.5"]))


def test_headers_declare_the_entries_and_argument_errors_come_back_by_name_without_a_device():
    import ctypes as C
    lib = _lib.load()
    for name in ("lt_sample_ode_cfg_rule", "lt_forward_cfg_rule", "lt_op_guidance_stats", "lt_op_unpatchify_cfg_rule", "lt_op_guidance_slices"):
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(lib, name), name
    assert lib.lt_op_guidance_slices() == 32
    a = _lib.LtStepArgs(batch=2, io_dtype=_lib.LT_BF16)
    grid = (C.c_float * 2)(0.0, 1.0)
    one = C.c_void_p(64)  # never dereferenced: every call below is refused before it reads anything
    assert lib.lt_sample_ode_cfg_rule(one, one, None, one, grid, 2, 0, None, 0.5, 1.0, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_cfg_rule: null argument" in lib.lt_last_error()
    assert lib.lt_forward_cfg_rule(None, one, one, one, 0.5, 1.0, C.byref(a), None) != 0
    assert b"lt_forward_cfg_rule: null argument" in lib.lt_last_error()
    assert lib.lt_op_guidance_stats(one, 40, 3, 8, 6, 10, 2, one, 3, 0, one, None) != 0 and b"even" in lib.lt_last_error()
    assert lib.lt_op_unpatchify_cfg_rule(one, 40, one, 1, 1024, 4, 8, 6, 10, 2, 1, one, 3, 0, 0, one, one, one, None, None) != 0
    assert b"256" in lib.lt_last_error()
