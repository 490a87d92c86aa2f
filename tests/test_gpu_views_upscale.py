"""-m gpu: Phase Upscale of multi-view (visual-anagram) sampling - the guided view gather word for word against the reference's tensor
expressions, lt_sample_views_guided against a host loop at the same batch, the reference's trajectories (tests/golden/views_upscale_tiny.npz,
full_2b_views_upscale_mid2.npz; made by scripts/make_views_upscale_golden.py from the unmodified reference), the softmax-rule plumbing, the
refusals and the sample_anagram driver with --upscale.

Gate against the reference (the project's standing rule): rel_l2(engine, fp32 reference) <= 1.5 x the smallest rel_l2 of the bf16 realisations of
the reference stored in the fixture, at every stored grid point."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models, views
from lumina_t2x_amd.engine import DiTEngine, EngineLimits, ffn_hidden_dim
from lumina_t2x_amd.transport.integrators import views_guided_table
from oracle import synth

import views_upscale_ref as UR
from gpu_util import P, lib, rel_l2, stream

pytestmark = pytest.mark.gpu

DT = {torch.float32: _lib.LT_F32, torch.bfloat16: _lib.LT_BF16}
CASES = ["up_v2", "up_v3", "up_v1r", "up_part"]
ANAGRAM, T2I = _lib.LT_SOFTMAX_ANAGRAM, _lib.LT_SOFTMAX_T2I


def _bf(bits):
    return torch.from_numpy(bits.copy()).view(torch.bfloat16)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = np.load(os.path.join(golden_dir, "views_upscale_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    m = models.NextDiT(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=True)
    return g, cfg, m.eval().to("cuda", torch.bfloat16)


def _case(g, name, dtype=torch.bfloat16):
    vnames, vargs = json.loads(str(g[f"{name}_views"]))
    torch.manual_seed(int(g[f"{name}_view_seed"]))
    vws = views.get_anagrams_views(vnames, view_args=vargs)
    caps, mask = _bf(g[f"{name}_caps"]).cuda(), torch.from_numpy(g[f"{name}_mask"]).cuda()
    z, guidance = torch.from_numpy(g[f"{name}_z"]).to("cuda", dtype), torch.from_numpy(g[f"{name}_guidance"]).to("cuda", dtype)
    assert np.array_equal(views.stack_tables(vws, z.shape[2], z.shape[3])[0].numpy(), g[f"{name}_perm"])
    return vws, caps, mask, z, guidance, json.loads(str(g[f"{name}_kwargs"]))


def _gather(y, G, Z, tabs, f0, half_dt, coef, dtype):
    perm_d, vs_d, is_d = tabs
    V, (Cc, h, w) = perm_d.shape[0], y.shape
    out = torch.full((V, Cc, h, w), float("nan"), dtype=dtype, device="cuda")
    arr = (C.c_float * 4)(*[float(v) for v in coef])
    _lib.check(lib().lt_op_views_guided_gather(P(y), P(G), P(Z), P(perm_d), P(vs_d), P(is_d), P(f0), P(out), float(half_dt), arr, V, Cc, h * w,
                                               DT[dtype], stream()), "lt_op_views_guided_gather")
    torch.cuda.synchronize()
    return out


def _view_sets(h, w):
    torch.manual_seed(h * 100 + w)
    sets = [[views.FlipView()], [views.NegateView(), views.PermuteView(torch.randperm(h * w))], [views.IdentityView(), views.NegateView(), views.Rotate180View()]]
    if h == w:
        sets += [[views.PatchPermuteView(4), views.Rotate90CWView()], [views.NegateView(), views.PatchPermuteView(4), views.Rotate90CCWView()]]
    return sets


@pytest.mark.parametrize("h, w", [(16, 16), (24, 32), (8, 12)])
def test_guided_gather_equals_the_reference_expressions_word_for_word(h, w):
    """generate.py:239-258 evaluated by torch on the GPU with fp32 scalars, views applied through lumina_t2x_amd.views: torch.equal at bf16 and
    fp32 states, both stages, V = 1, 2, 3 (negate, patch_permute and a random permutation among them).  Also reports what the literal
    expression with the 0-dim CPU tensor c gives on this device (the form the public default assumes; nothing is asserted on it)."""
    Cc = 4
    g = torch.Generator().manual_seed(h * 1000 + w)
    literal = {"fp32": 0, "state": 0, "neither": 0}
    for vs_list in _view_sets(h, w):
        perm, vsign, isign = views.stack_tables(vs_list, h, w, Cc)
        tabs = (perm.cuda(), vsign.cuda(), isign.cuda())
        V = len(vs_list)
        for dtype in (torch.bfloat16, torch.float32):
            y, G, Z = (torch.randn(Cc, h, w, generator=g).to(dtype).cuda() for _ in range(3))
            f0 = torch.randn(V, Cc, h, w, generator=g).to(dtype).cuda()
            for t, half_dt in ((0.0, 0.05), (0.13, 0.0685), (0.37, 0.12), (0.71, 0.031), (0.93, 0.035), (1.0, 0.0)):
                t = float(torch.tensor(t, dtype=torch.float32))  # a grid point is an fp32 value
                coef = {form: views_guided_table([t, 1.0], dtype, form)[0, 0] for form in ("fp32", "state")}
                sc = UR.expression_scalars(t, "float")
                assert [float(v) for v in coef["fp32"]] == [sc[0], sc[1], sc[2], sc[3]]
                for stage_f0 in (None, f0):
                    got = _gather(y, G, Z, tabs, stage_f0, half_dt, coef["fp32"], dtype)
                    want = UR.expression_input(y, G, Z, stage_f0, half_dt, sc, vs_list)
                    assert torch.equal(got, want), (h, w, V, dtype, t, stage_f0 is not None)
                    assert torch.equal(got, UR.chain_input(y, G, Z, stage_f0, half_dt, coef["fp32"], vs_list, dtype))
                    if dtype == torch.bfloat16 and 0.0 < t < 1.0:
                        lit = UR.expression_input(y, G, Z, stage_f0, half_dt, UR.expression_scalars(t, "tensor"), vs_list)
                        st = _gather(y, G, Z, tabs, stage_f0, half_dt, coef["state"], dtype)
                        literal["fp32" if torch.equal(lit, got) else ("state" if torch.equal(lit, st) else "neither")] += 1
    print(f"{h}x{w}: the literal expression (0-dim fp32 CPU tensor c times a bf16 device tensor) equals the kernel with coef_rounding "
          f"fp32 in {literal['fp32']} cases, state in {literal['state']}, neither in {literal['neither']}")


def test_guided_gather_on_bf16_ties_and_without_fma():
    """coefficients are data: with kc = k1c = 0.5, ft = 1, f1t = 0 the sum R(k1c s) + R(kc g) of chosen bf16 values lands exactly between two
    bf16 numbers (round to even both ways); at an fp32 state a fused multiply-add anywhere in the chain would change words - shown on the CPU first"""
    h, w, Cc = 8, 12, 4
    vs_list = [views.FlipView(), views.NegateView()]
    perm, vsign, isign = views.stack_tables(vs_list, h, w, Cc)
    tabs = (perm.cuda(), vsign.cuda(), isign.cuda())
    # ties: 0.5 * 2 + 0.5 * 2^-7 = 1 + 2^-8 (-> 1, even), 0.5 * (2 + 2^-6) + 0.5 * 2^-7 = 1 + 2^-7 + 2^-8 (-> 1 + 2^-6, even), both signs
    y = torch.full((Cc, h, w), 2.0)
    y[1] = 2.0 + 2.0 ** -6
    y[2] = -2.0
    y[3] = -(2.0 + 2.0 ** -6)
    G = torch.full((Cc, h, w), 2.0 ** -7)
    G[2:] = -(2.0 ** -7)
    yb, Gb = y.to(torch.bfloat16).cuda(), G.to(torch.bfloat16).cuda()
    assert torch.equal(yb.float().cpu(), y) and torch.equal(Gb.float().cpu(), G)
    coef = (1.0, 0.0, 0.5, 0.5)
    exact = 0.5 * y.double() + 0.5 * G.double()
    assert not torch.equal(exact.to(torch.bfloat16).double(), exact)  # the exact sum is no bf16 number ...
    lo, hi = exact.float().view(torch.int32) & ~0xFFFF, (exact.float().view(torch.int32) & ~0xFFFF) + 0x10000
    assert torch.equal(exact - lo.view(torch.float32).double(), hi.view(torch.float32).double() - exact)  # ... but the midpoint of its neighbours
    got = _gather(yb, Gb, torch.zeros_like(Gb), tabs, None, 0.0, coef, torch.bfloat16)
    want = UR.expression_input(yb, Gb, torch.zeros_like(Gb), None, 0.0, coef, vs_list)
    assert torch.equal(got, want)
    assert torch.equal(got[1, 0].float().cpu(), torch.full((h, w), -1.0)) and torch.equal(got[1, 1].float().cpu(), torch.full((h, w), -(1.0 + 2.0 ** -6)))
    # fp32 state: unfused against every single fused form, on the CPU first
    g = torch.Generator().manual_seed(77)
    y, G, Z = (torch.randn(Cc, h, w, generator=g) for _ in range(3))
    f0 = torch.randn(2, Cc, h, w, generator=g)
    coef = [float(v) for v in views_guided_table([0.37, 1.0], torch.float32, "fp32")[0, 0]]
    half_dt = 0.0685
    ft, f1t, kc, k1c = (torch.tensor(v, dtype=torch.float32) for v in coef)
    fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()  # one rounding (the double product of two floats is exact)
    gsum = ft * G + f1t * Z
    unfused = k1c * y + kc * gsum
    assert not torch.equal(fma(k1c, y, kc * gsum), unfused) and not torch.equal(fma(kc, gsum, k1c * y), unfused)
    assert not torch.equal(fma(ft, G, f1t * Z), gsum) and not torch.equal(fma(f1t, Z, ft * G), gsum)
    hd = torch.tensor(half_dt, dtype=torch.float32)
    assert not torch.equal(fma(f0[0], hd, y), y + f0[0] * hd)
    for stage_f0 in (None, f0):
        want = UR.chain_input(y, G, Z, stage_f0, half_dt, coef, vs_list, torch.float32)  # CPU, unfused
        got = _gather(y.cuda(), G.cuda(), Z.cuda(), tabs, None if stage_f0 is None else stage_f0.cuda(), half_dt, coef, torch.float32)
        assert torch.equal(got.cpu(), want)
        assert torch.equal(got, UR.expression_input(y.cuda(), G.cuda(), Z.cuda(), None if stage_f0 is None else stage_f0.cuda(), half_dt, coef, vs_list))
    assert torch.equal(UR.chain_input(y, G, Z, None, 0.0, coef, [views.IdentityView()], torch.float32)[0], unfused)


def _engine_for(model, vws, caps, mask, z):
    V = len(vws)
    eng = model.engine(z.expand(2 * V, -1, -1, -1), caps.shape[1])
    eng.prepare_prompt(caps, mask)
    eng.set_views(vws, z.shape[2], z.shape[3])
    return eng


def _batched_fwd(eng, V, cfg_scale, kw):
    """one forward_with_cfg of 2 V rows per stage (rows V..2V-1 are replaced by the first half inside the call)"""
    def fwd(x, t, stage):
        return eng.forward(torch.cat([x, x]).contiguous(), torch.full((2 * V,), t), use_cfg=True, cfg_scale=cfg_scale, scale_watershed=0.0, **kw)[:V]
    return fwd


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", CASES)
def test_sampler_equals_a_host_loop_at_the_same_batch(tiny, name, dtype):
    """lt_sample_views_guided against a Python loop over the same engine: the reference's expressions with fp32 scalars for the model inputs,
    one forward_with_cfg of 2 V rows per stage, the closing update in the order views_reduce states (tests/test_gpu_views.py pins that
    kernel to it word for word; torch's own stack(...).mean(0) may differ from it by one ulp on the device)"""
    g, cfg, model = tiny
    vws, caps, mask, z, guidance, kw = _case(g, name, dtype)
    grid = [float(v) for v in g["grid"]]
    V = len(vws)
    eng = _engine_for(model, vws, caps, mask, z)
    eng.set_softmax_rule(ANAGRAM)
    try:
        coef = views_guided_table(grid, dtype, "fp32")
        traj = eng.sample_views_guided(z, guidance, grid, coef, cfg_scale=float(g["cfg_scale"]), scale_watershed=0.0, **kw)
        assert eng.last_nfe() == 2 * (len(grid) - 1)
        fin = eng.sample_views_guided(z, guidance, grid, coef, noise=z.clone(), cfg_scale=float(g["cfg_scale"]), scale_watershed=0.0,
                                      return_trajectory=False, **kw)
        want = UR.expression_loop(_batched_fwd(eng, V, float(g["cfg_scale"]), kw), vws, z, guidance, z, grid, "float",
                                  close=lambda y, f1, dt: UR.chain_close(y, f1, dt, vws, dtype))
    finally:
        eng.set_softmax_rule(T2I)
    assert traj.shape == want.shape == (len(grid),) + tuple(z.shape[1:]) and torch.isfinite(traj.float()).all()
    for k in range(len(grid)):
        assert torch.equal(traj[k], want[k]), (name, dtype, k)
    assert torch.equal(fin[0], traj[-1]) and not torch.equal(traj[1], traj[0])


def _gate(name, traj, ref, realisations):
    """the standing rule at every grid point: engine vs fp32 reference <= 1.5 x min over the stored bf16 realisations; prints both"""
    worst = []
    for k in range(1, ref.shape[0]):
        e = rel_l2(traj[k], ref[k])
        fl = {n: rel_l2(r[k], ref[k]) for n, r in realisations.items()}
        floor = min(fl.values())
        print(f"{name} grid point {k}: engine vs fp32 reference {e:.3e} | floor {floor:.3e} ({', '.join(f'{n} {v:.3e}' for n, v in fl.items())}) "
              f"| ratio {e / floor:.2f}")
        worst.append((k, e, floor))
    for k, e, floor in worst:
        assert e <= 1.5 * floor, (name, k, e, floor)


@pytest.mark.parametrize("name", CASES)
def test_tiny_trajectories_against_the_reference(tiny, name):
    g, cfg, model = tiny
    vws, caps, mask, z, guidance, kw = _case(g, name)
    grid = torch.from_numpy(g["grid"])
    traj = model.sample_views_guided(z, guidance, grid, vws, caps, mask, cfg_scale=float(g["cfg_scale"]), coef_rounding=str(g["c_rounding"]),
                                     scale_watershed=0.7, **kw)
    ref = torch.from_numpy(g[f"{name}_ref"])
    assert traj.shape == ref.shape and model._engine.last_nfe() == 2 * (len(grid) - 1)
    assert model._engine.softmax_rule == T2I  # restored
    _gate(f"views_upscale_tiny/{name}", traj.float().cpu(), ref, {"plain": _bf(g[f"{name}_refbf16"]).float(), "autocast": _bf(g[f"{name}_refbf16ac"]).float()})


def _full_inputs(g, cfg):
    """z, guidance and prompts of the full-depth case, regenerated from the seed as scripts/make_views_upscale_golden.py drew them"""
    case = json.loads(str(g["case"]))
    rng = np.random.default_rng(case["seed_x"])
    L, lens, neg = case["latent"], case["lens"], int(g["neg_len"])
    draw = lambda: torch.from_numpy(rng.standard_normal((1, cfg.in_channels, L, L), dtype=np.float32)).to(torch.bfloat16)
    z, guidance = draw(), draw()
    V = len(lens)
    T = (max(lens + [neg]) + 7) // 8 * 8
    caps = torch.zeros(2 * V, T, cfg.cap_feat_dim)
    mask = torch.zeros(2 * V, T, dtype=torch.int32)
    negf = torch.from_numpy(rng.standard_normal((neg, cfg.cap_feat_dim), dtype=np.float32))
    for v, n in enumerate(lens):
        caps[v, :n] = torch.from_numpy(rng.standard_normal((n, cfg.cap_feat_dim), dtype=np.float32))
        mask[v, :n] = 1
        caps[V + v, :neg] = negf
        mask[V + v, :neg] = 1
    pad = torch.from_numpy(rng.standard_normal((2 * V, T, cfg.cap_feat_dim), dtype=np.float32))
    caps = torch.where(mask.bool().unsqueeze(-1), caps, pad).to(torch.bfloat16)
    assert np.array_equal(z.float().flatten()[:8].numpy(), g["z_probe"]) and np.array_equal(guidance.float().flatten()[:8].numpy(), g["guidance_probe"])
    assert np.array_equal(caps.float().flatten()[:8].numpy(), g["caps_probe"])
    return case, z, guidance, caps, mask


def test_full_2b_two_views_guided_2_intervals_against_the_reference(golden_dir, tiny):
    """NextDiT_2B_patch2, all 24 layers, the anagram attention rule, latent 64 x 64 (1024 tokens, 4 query chunks of base_seqlen 256),
    scale_factor 2, views identity + rotate_cw, 2 guided midpoint intervals: against the unmodified reference's loop, model and views in fp32;
    floor = its own bf16 runs (plain, autocast)"""
    g = np.load(os.path.join(golden_dir, "full_2b_views_upscale_mid2.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    case = json.loads(str(g["case"]))
    sd = synth.synth_state_dict(cfg, seed=case["seed_w"], streams=True)
    keys = json.loads(str(g["wkeys"]))
    wsum = np.array([float(sd[k].double().abs().sum()) for k in keys[:3]])
    if not (np.allclose(wsum, g["wsum"], rtol=1e-12) and np.array_equal(sd[keys[3]].flatten()[:8].double().numpy(), g["wprobe"])):
        pytest.skip("the seeded weight draw does not reproduce on this numpy: a live CPU trajectory at full depth would take an hour")
    model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=cfg.cap_feat_dim)
    model.load_state_dict(sd, strict=True)
    model = model.eval().to("cuda", torch.bfloat16)
    del sd
    case, z, guidance, caps, mask = _full_inputs(g, cfg)
    vws = views.get_anagrams_views(case["views"])
    traj = model.sample_views_guided(z.cuda(), guidance.cuda(), torch.from_numpy(g["grid"]), vws, caps.cuda(), mask.cuda(), cfg_scale=float(g["cfg_scale"]),
                                     coef_rounding=str(tiny[0]["c_rounding"]), **case["kwargs"])
    assert model._engine.last_nfe() == 2 * case["intervals"]
    _gate("full_2b_views_upscale_mid2", traj.float().cpu(), torch.from_numpy(g["ref"]),
          {"plain": _bf(g["refbf16"]).float(), "autocast": _bf(g["refbf16ac"]).float()})
    del model
    torch.cuda.empty_cache()


def test_softmax_rule_plumbing_and_graph_key(tiny):
    g, cfg, model = tiny
    vws, caps, mask, z, guidance, kw = _case(g, "up_v2")
    x = torch.from_numpy(g["up_v2_fwd_x"]).to("cuda", torch.bfloat16)
    x = torch.stack([x, x])
    t = torch.full((2,), float(g["up_v2_fwd_t"]))
    pair = (caps[[0, 2]].contiguous(), mask[[0, 2]].contiguous())
    eng = model.engine(x, caps.shape[1])
    eng.set_option("graph", 1)  # replay at every size: the rule must be part of the key
    try:
        eng.prepare_prompt(*pair)
        call = lambda **k: eng.forward(x, t, use_cfg=True, cfg_scale=float(g["cfg_scale"]), scale_watershed=0.0, **dict(kw, **k))

        def under(rule, n=3):
            eng.set_softmax_rule(rule)
            outs = [call() for _ in range(n)]  # eager, capture + replay, replay
            assert all(torch.equal(o, outs[0]) for o in outs)
            return outs[0]

        r0 = eng.graph_replays()
        first = under(T2I)
        assert eng.graph_replays() >= r0 + 2
        ana = under(ANAGRAM)
        r1 = eng.graph_replays()
        third = under(T2I, 1)
        assert eng.graph_replays() == r1 + 1  # served by the graph captured under T2I ...
        assert torch.equal(third, first) and not torch.equal(ana, first)  # ... never by the one captured under the other rule
        assert torch.equal(under(ANAGRAM, 1), ana)
        # against the fork's own output at this input (fp32 module), floor = the bf16 module on the same input
        ref = torch.from_numpy(g["up_v2_fwd_out"])
        floor = min(rel_l2(_bf(g[f"up_v2_fwd_out{s}"]).float(), ref) for s in ("bf16", "bf16ac"))
        e_ana, e_t2i = rel_l2(ana[0], ref), rel_l2(first[0], ref)
        print(f"forward_with_cfg on up_v2's shape vs the fork in fp32: anagram rule {e_ana:.3e}, T2I rule {e_t2i:.3e}, floor {floor:.3e}")
        assert e_ana <= 1.5 * floor
        # without proportional attention both rules are sqrt(1 / hd)
        eng.set_softmax_rule(T2I)
        plain = call(proportional_attn=False, base_seqlen=None)
        eng.set_softmax_rule(ANAGRAM)
        assert torch.equal(call(proportional_attn=False, base_seqlen=None), plain)
    finally:
        eng.set_softmax_rule(T2I)
        eng.set_option("graph", None)


def _raw(eng, z, guidance, coef, grid, a, traj=None):
    garr = (C.c_float * len(grid))(*grid)
    coef = coef.contiguous()
    rc = eng.lib.lt_sample_views_guided(eng.handle, P(z), P(guidance), P(z), P(traj), P(None), garr, C.cast(coef.data_ptr(), C.POINTER(C.c_float)),
                                        len(grid), C.byref(a), stream())
    return rc, eng.lib.lt_last_error().decode()


def test_refusals_by_name(tiny):
    g, cfg, model = tiny
    vws, caps, mask, z, guidance, kw = _case(g, "up_v2")
    grid = [float(v) for v in g["grid"]]
    coef = views_guided_table(grid, z.dtype, "fp32")
    eng = _engine_for(model, vws, caps, mask, z)
    a = eng._step_args(z, 4.0, 1.0, 0.0, None, False)
    traj = torch.full((len(grid),) + tuple(z.shape[1:]), 7.0, dtype=z.dtype, device="cuda")
    a.batch = 2  # V = 2 needs 4
    rc, msg = _raw(eng, z, guidance, coef, grid, a, traj)
    assert rc != 0 and "need a->batch = 2 V = 4" in msg
    a.batch = 4
    rc, msg = _raw(eng, z, guidance, coef, grid[:1], a, traj)
    assert rc != 0 and "at least 2 grid points" in msg
    with pytest.raises(_lib.LuminaLibError, match="view tables are for a 32x32 latent, the call has 16x16"):
        eng.sample_views_guided(z[:, :, :16, :16].contiguous(), guidance[:, :, :16, :16].contiguous(), grid, coef)
    bad = coef.clone()
    bad[1, 1, 2] = float("nan")
    with pytest.raises(_lib.LuminaLibError, match="coefficient 2 of stage 1 \\(interval 1\\) is not finite"):
        eng.sample_views_guided(z, guidance, grid, bad, cfg_scale=4.0)
    bad[1, 1, 2] = float("inf")
    rc, msg = _raw(eng, z, guidance, bad, grid, a, traj)
    assert rc != 0 and "not finite" in msg
    with pytest.raises(_lib.LuminaLibError, match="unknown softmax rule 7"):
        eng.set_softmax_rule(7)
    with pytest.raises(_lib.LuminaLibError, match="not in"):
        eng.set_softmax_rule("fork")
    eng.set_views(None, 0, 0)
    rc, msg = _raw(eng, z, guidance, coef, grid, a, traj)
    assert rc != 0 and "no view tables" in msg
    with pytest.raises(_lib.LuminaLibError, match="no views uploaded"):
        eng.sample_views_guided(z, guidance, grid, coef)
    torch.cuda.synchronize()
    assert bool((traj == 7.0).all())  # no refused call wrote a partial result
    # a shape the fork's query chunks do not cover: 12 x 86 latent = 258 tokens, base_seqlen 256 (the fixture records what the module does)
    print(f"the unmodified module on {str(g['chunk_gap_case'])}: {str(g['chunk_gap_result'])}")
    gap = json.loads(str(g["chunk_gap_case"]))
    H, W = gap["latent"]
    zg = torch.randn(1, 4, H, W, device="cuda").to(torch.bfloat16)
    one = [views.IdentityView()]
    cap1, mask1 = caps[[0, 2]].contiguous(), mask[[0, 2]].contiguous()
    with pytest.raises(_lib.LuminaLibError, match="do not cover 258 tokens"):
        model.sample_views_guided(zg, zg.clone(), grid, one, cap1, mask1, proportional_attn=True, base_seqlen=gap["base_seqlen"])
    eng = model._engine
    assert eng.softmax_rule == T2I
    tt = torch.full((2,), 0.3)
    out = eng.forward(zg.repeat(2, 1, 1, 1), tt, use_cfg=True, cfg_scale=4.0, proportional_attn=True, base_seqlen=gap["base_seqlen"])  # T2I rule: served
    assert torch.isfinite(out.float()).all()
    eng.set_softmax_rule(ANAGRAM)
    try:
        with pytest.raises(_lib.LuminaLibError, match="do not cover 258 tokens"):
            eng.forward(zg.repeat(2, 1, 1, 1), tt, use_cfg=True, cfg_scale=4.0, proportional_attn=True, base_seqlen=gap["base_seqlen"])
        eng.forward(zg.repeat(2, 1, 1, 1), tt, use_cfg=True, cfg_scale=4.0)  # no proportional attention: nothing to refuse
    finally:
        eng.set_softmax_rule(T2I)
    # any other variant is refused by name, before anything is launched
    other = DiTEngine(variant=_lib.LT_VARIANT_NEXT_IMAGENET, dim=384, n_layers=2, n_heads=8, n_kv_heads=8, ffn_hidden=ffn_hidden_dim(384, 256, None),
                      patch_size=2, in_channels=4, out_channels=8, cap_feat_dim=0, qk_norm=True, norm_eps=1e-5, num_classes=10,
                      limits=EngineLimits(4, 256, 256))
    with pytest.raises(_lib.LuminaLibError, match="LT_VARIANT_NEXT_T2I"):
        other.set_softmax_rule(ANAGRAM)
    rc, msg = _raw(other, z, guidance, coef, grid, a, traj)
    assert rc != 0 and "LT_VARIANT_NEXT_T2I" in msg
    rc = other.lib.lt_sample_views_guided(other.handle, P(z), P(None), P(z), P(None), P(None), None, None, 4, C.byref(a), stream())
    assert rc != 0 and b"null argument" in other.lib.lt_last_error()


@pytest.mark.parametrize("res, latent", [("128:128x128", 16), ("256:256x256", 32)])
def test_sample_anagram_upscale_end_to_end(tiny, tmp_path, res, latent):
    from lumina_t2x_amd import sample_anagram
    g, cfg, model = tiny

    def encode(captions):  # a stand-in text encoder: features seeded by the caption, lengths differ, padded to a multiple of 8
        lens = [3 + len(c) % 9 for c in captions]
        T = (max(lens) + 7) // 8 * 8
        feats = torch.zeros(len(captions), T, cfg.cap_feat_dim)
        mask = torch.zeros(len(captions), T, dtype=torch.int32)
        for i, (c, n) in enumerate(zip(captions, lens)):
            gen = torch.Generator().manual_seed(sum(map(ord, c)))
            feats[i] = torch.randn(T, cfg.cap_feat_dim, generator=gen)
            mask[i, :n] = 1
        return feats.to("cuda", torch.bfloat16), mask.cuda()

    def decode(lat):  # a stand-in VAE decoder: 8 x nearest upsampling of three channels into [0, 1]
        return torch.sigmoid(torch.nn.functional.interpolate(lat[:, :3].float(), scale_factor=8, mode="nearest"))

    def vae_encode(img):  # a stand-in VAE encoder: 8 x average pooling, the fourth channel the mean of the three
        p = torch.nn.functional.avg_pool2d(img.float(), 8)
        return torch.cat([p, p.mean(dim=1, keepdim=True)], dim=1) * 4.0

    args = sample_anagram.build_parser().parse_args(
        ["--name", "t", "--save_dir", str(tmp_path), "--prompts", "a duck", "a rabbit", "--views", "identity", "rotate_cw", "--style", "a painting of",
         "--num_inference_steps", "4", "--time_shifting_factor", "4", "--cfg_scale", "4", "--seed", "3", "--resolution", res, "--upscale"])
    targs = types.SimpleNamespace(image_size=128, vae="sdxl")
    info = sample_anagram.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode, model=model, train_args=targs,
                              vae_encode_fn=vae_encode)
    assert len(info) == 1 and model._engine.last_nfe() == 2 * 3
    lat = torch.load(info[0]["upscaled_latent"])
    assert lat.shape == (1, 4, latent, latent) and torch.isfinite(lat.float()).all()
    # what the driver did, by hand
    cat = int(res.split(":")[0])
    torch.manual_seed(3)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16)
    feats, mask = sample_anagram.encode_views(encode, ["a duck", "a rabbit"], "a painting of", args.negative_prompt)
    vws = views.get_anagrams_views(["identity", "rotate_cw"])
    grid = sample_anagram.time_grid(4, 4.0)
    init = model.sample_views(z, grid, vws, feats, mask, "midpoint", cfg_scale=4.0, return_trajectory=False)
    assert torch.equal(torch.load(info[0]["latent"]), init.cpu())
    img = torch.nn.functional.interpolate(decode(init / 0.13025).float() * 2 - 1, size=(cat, cat), mode="bicubic").to(torch.bfloat16)
    guidance = (vae_encode(img) * 0.13025).to(torch.bfloat16)
    z2 = torch.randn_like(guidance)
    kw = dict(proportional_attn=True, base_seqlen=64, scale_factor=2.0 if cat > 128 else 1.0)
    assert info[0]["upscale"] == kw
    want = model.sample_views_guided(z2, guidance, grid, vws, feats, mask, cfg_scale=4.0, return_trajectory=False, **kw)
    assert torch.equal(lat, want.cpu())
    for key in ("image", "views_image", "upscaled_image", "upscaled_views_image"):
        assert os.path.getsize(info[0][key]) > 0
