"""-m gpu: multi-view (visual-anagram) sampling - the three view kernels against torch indexing, lt_set_views' refusals, lt_sample_views
against lt_sample_ode (degenerate case), against the reference's trajectories (tests/golden/views_tiny.npz, full_2b_views_mid4.npz; made by
scripts/make_views_golden.py from the unmodified reference) and against the same loop driven from Python one view at a time, and the
sample_anagram driver end to end.

Gate against the reference (the project's standing rule, tests/test_gpu_fulldepth.py): rel_l2(engine, fp32 reference) <= 1.5 x the smallest
rel_l2 of the bf16 realisations of the reference stored in the fixture, at every grid point and at the end."""
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
from oracle import synth

from gpu_util import P, lib, rel_l2, stream

pytestmark = pytest.mark.gpu

DT = {torch.float32: _lib.LT_F32, torch.bfloat16: _lib.LT_BF16}


def _bf(bits):
    return torch.from_numpy(bits.copy()).view(torch.bfloat16)


def _views_for(h, w, V, seed):
    """V views cycling through every built view this latent admits, plus a caller-supplied random permutation"""
    torch.manual_seed(seed)
    pool = [views.IdentityView(), views.FlipView(), views.NegateView(), views.PermuteView(torch.randperm(h * w)), views.Rotate180View()]
    if h == w:
        pool += [views.Rotate90CWView(), views.Rotate90CCWView(), views.PatchPermuteView(4)]
        if h % 64 == 0:
            pool.append(views.get_anagrams_views(["pixel_permute"])[0])
    return pool


def _invert(perm):
    V, HW = perm.shape
    iperm = torch.empty_like(perm)
    hits = torch.full((V * HW + 1,), 7, dtype=torch.int32, device="cuda")
    _lib.check(lib().lt_op_views_invert(P(perm), P(iperm), P(hits), V, HW, stream()), "lt_op_views_invert")
    torch.cuda.synchronize()
    return iperm, hits


@pytest.mark.parametrize("h, w", [(16, 16), (64, 64), (128, 128), (32, 48)])
def test_view_kernels_against_torch_indexing(h, w):
    """invert and gather bit-exact for every built view; reduce bit-exact against the stated order (fp32 sum over v = 0..V-1, one division,
    one rounding, subtract, one rounding) and within one bf16 ulp of torch's own stack(...).mean(0) form"""
    Cc, HW = 4, h * w
    pool = _views_for(h, w, 4, 3)
    g = torch.Generator().manual_seed(h * 1000 + w)
    for V in (1, 2, 3, 4):
        for start in range(0, len(pool), 2):
            vs_list = [pool[(start + k) % len(pool)] for k in range(V)]
            perm, vsign, isign = views.stack_tables(vs_list, h, w, Cc)
            perm_d, vs_d, is_d = perm.cuda(), vsign.cuda(), isign.cuda()
            iperm_d, hits = _invert(perm_d)
            want_inv = torch.empty_like(perm)
            for v in range(V):
                want_inv[v, perm[v].long()] = torch.arange(HW, dtype=torch.int32)
            assert torch.equal(iperm_d.cpu(), want_inv)
            assert int(hits[-1]) == 0 and bool((hits[:-1] == 1).all())
            for dtype in (torch.bfloat16, torch.float32):
                y = torch.randn(Cc, h, w, generator=g).to(dtype)
                f = torch.randn(V, Cc, h, w, generator=g).to(dtype)
                yd, fd = y.cuda(), f.cuda()
                dt, half_dt = 0.137, 0.0685
                dt_t, hdt_t = torch.tensor(dt, dtype=torch.float32), torch.tensor(half_dt, dtype=torch.float32)
                R = (lambda x: x.to(torch.bfloat16).float()) if dtype == torch.bfloat16 else (lambda x: x)
                # gather: against the classes' own view() (torch ops) - bit-exact
                out = torch.full((V, Cc, h, w), float("nan"), dtype=dtype, device="cuda")
                _lib.check(lib().lt_op_views_gather(P(yd), P(perm_d), P(vs_d), P(None), P(out), 0.0, V, Cc, HW, DT[dtype], stream()), "gather")
                x_want = torch.stack([vw.view(y) for vw in vs_list])
                assert torch.equal(out.cpu(), x_want), (h, w, V, dtype)
                # gather, midpoint stage: x + f0 * half_dt as torch computes it on tensors of this dtype (Python-float scalar: fp32 multiply)
                _lib.check(lib().lt_op_views_gather(P(yd), P(perm_d), P(vs_d), P(fd), P(out), half_dt, V, Cc, HW, DT[dtype], stream()), "gather mid")
                mid_want = R(x_want.float() + R(f.float() * hdt_t)).to(dtype)
                assert torch.equal(out.cpu(), mid_want), (h, w, V, dtype)
                assert torch.equal(mid_want, x_want + f * half_dt)  # ... which IS the reference's expression (generate.py:217)
                # reduce
                red = torch.full((Cc, h, w), float("nan"), dtype=dtype, device="cuda")
                _lib.check(lib().lt_op_views_reduce(P(yd), P(fd), P(iperm_d), P(is_d), P(red), dt, V, Cc, HW, DT[dtype], stream()), "reduce")
                noises = [vw.inverse_view(-(f[v] * dt)) for v, vw in enumerate(vs_list)]  # generate.py:402-407 on tensors of this dtype
                acc = torch.zeros(Cc, h, w)
                for n in noises:
                    acc = acc + n.float()
                stated = R(y.float() - R(acc / V)).to(dtype)
                assert torch.equal(red.cpu(), stated), (h, w, V, dtype)
                torch_form = (y - torch.stack(noises).mean(dim=0)).float()  # generate.py:410-414
                if dtype == torch.bfloat16:  # one bf16 ulp (2^-7 relative at most) at the magnitude of the subtraction's operands
                    mean_t = torch.stack(noises).mean(dim=0).float().abs()
                    ulp = torch.maximum(torch.maximum(y.float().abs(), mean_t), torch_form.abs()) * 2.0 ** -7
                    assert bool(((red.cpu().float() - torch_form).abs() <= ulp).all()), (h, w, V)
                else:
                    assert torch.allclose(red.cpu(), torch_form, rtol=1e-6, atol=1e-6)


def test_invert_counts_a_table_that_is_not_a_bijection():
    perm = torch.stack([torch.randperm(256), torch.randperm(256)]).to(torch.int32)
    perm[1, 5] = perm[1, 9]      # names a target twice
    perm[0, 3] = 256             # out of range
    perm[0, 4] = -1
    _, hits = _invert(perm.cuda())
    assert int(hits[-1]) == 3


def _tiny_model(golden_dir):
    g = np.load(os.path.join(golden_dir, "views_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    m = models.NextDiT(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=True)
    return g, cfg, m.eval().to("cuda", torch.bfloat16)


def _tiny_case(g, name):
    vnames, vargs = json.loads(str(g[f"{name}_views"]))
    torch.manual_seed(int(g[f"{name}_view_seed"]))
    vws = views.get_anagrams_views(vnames, view_args=vargs)
    caps, mask, z = _bf(g[f"{name}_caps"]).cuda(), torch.from_numpy(g[f"{name}_mask"]).cuda(), torch.from_numpy(g[f"{name}_z"])
    assert np.array_equal(views.stack_tables(vws, z.shape[2], z.shape[3])[0].numpy(), g[f"{name}_perm"])
    return vws, caps, mask, z.to("cuda", torch.bfloat16)


def test_set_views_and_sample_views_refusals(golden_dir):
    g, cfg, model = _tiny_model(golden_dir)
    vws, caps, mask, z = _tiny_case(g, "v2")
    eng = model.engine(z.expand(4, -1, -1, -1), caps.shape[1])
    eng.prepare_prompt(caps, mask)
    perm, vs, isg = views.stack_tables(vws, 16, 16)
    bad = perm.clone()
    bad[1, 7] = bad[1, 8]
    with pytest.raises(_lib.LuminaLibError, match="not a bijection"):
        eng.set_views((bad, vs, isg), 16, 16)
    with pytest.raises(_lib.LuminaLibError, match="no view"):  # the refused upload left no tables behind
        eng.sample_views(z, [0.0, 1.0])
    with pytest.raises(_lib.LuminaLibError, match="do not match a 16x18 latent"):
        eng.set_views((perm, vs, isg), 16, 18)
    with pytest.raises(_lib.LuminaLibError, match="multiple of the patch size"):
        eng.set_views((perm[:, :15 * 15], vs, isg), 15, 15)
    three = views.stack_tables(vws + [views.FlipView()], 16, 16)
    with pytest.raises(_lib.LuminaLibError, match="max_batch is 4"):
        eng.set_views(three, 16, 16)
    with pytest.raises(_lib.LuminaLibError, match=r"\+1 / -1"):
        eng.set_views((perm, vs * 0.5, isg), 16, 16)
    eng.set_views(vws, 16, 16)
    with pytest.raises(_lib.LuminaLibError, match="rk4"):
        eng.sample_views(z, [0.0, 0.5, 1.0], "rk4")
    with pytest.raises(_lib.LuminaLibError, match="16x16 latent, the call has 32x32"):
        eng.sample_views(torch.zeros(1, 4, 32, 32, device="cuda", dtype=torch.bfloat16), [0.0, 1.0])
    # the prompt must have been prepared at B = 2 V
    eng.prepare_prompt(caps[[0, 2]].contiguous(), mask[[0, 2]].contiguous())
    with pytest.raises(_lib.LuminaLibError, match="batch 2, step has batch 4"):
        eng.sample_views(z, [0.0, 1.0])
    # any other variant is refused by name, before anything is launched
    other = DiTEngine(variant=_lib.LT_VARIANT_NEXT_IMAGENET, dim=384, n_layers=2, n_heads=8, n_kv_heads=8, ffn_hidden=ffn_hidden_dim(384, 256, None),
                      patch_size=2, in_channels=4, out_channels=8, cap_feat_dim=0, qk_norm=True, norm_eps=1e-5, num_classes=10,
                      limits=EngineLimits(4, 64, 256))
    with pytest.raises(_lib.LuminaLibError, match="LT_VARIANT_NEXT_T2I"):
        other.set_views(vws, 16, 16)
    a = other._step_args(z.expand(4, -1, -1, -1), 4.0, 1.0, 1.0, None, False)
    grid = (C.c_float * 2)(0.0, 1.0)
    rc = other.lib.lt_sample_views(other.handle, P(z), P(None), P(z.clone()), grid, 2, _lib.LT_ODE_MIDPOINT, C.byref(a), stream())
    assert rc != 0 and b"LT_VARIANT_NEXT_T2I" in other.lib.lt_last_error()


@pytest.mark.parametrize("method", ["midpoint", "euler"])
def test_one_identity_view_is_lt_sample_ode_bit_for_bit(golden_dir, method):
    """V = 1, identity, grid 0, 1/4, 1/2, 3/4, 1 (dt, dt / 2 and the midpoints are exact in any arithmetic): the multi-view loop IS the plain ODE
    loop - gather = copy, reduce = y + dt f - so lt_sample_views must equal lt_sample_ode on the latent duplicated to batch 2, bit for bit"""
    g, cfg, model = _tiny_model(golden_dir)
    _, caps, mask, z = _tiny_case(g, "v1")
    grid = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])
    traj = model.sample_views(z, grid, [views.IdentityView()], caps, mask, method, cfg_scale=4.0)
    eng = model._engine
    assert eng.last_nfe() == 4 * (2 if method == "midpoint" else 1)
    eng.prepare_prompt(caps, mask)
    want = eng.sample_ode(z.repeat(2, 1, 1, 1), grid, method, use_cfg=True, cfg_scale=4.0, t_round_to_state_dtype=False)
    assert traj.shape == (5, 4, 16, 16) and torch.isfinite(traj.float()).all()
    assert torch.equal(traj, want[:, 0])
    assert not torch.equal(traj[1], traj[0])


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


def _sequential(model, vws, caps, mask, z, grid):
    """the reference's loop driven from Python on the engine's model callable: one forward_with_cfg of batch 2 per view and stage, torch
    view ops, torch arithmetic on bf16 tensors (generate.py:389-414, :212-219)"""
    V = len(vws)
    noisy = z.repeat(2, 1, 1, 1)
    states = [noisy[0].clone()]
    calls = 0
    pairs = [(caps[[v, V + v]].contiguous(), mask[[v, V + v]].contiguous()) for v in range(V)]
    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = t1 - t0
        half_dt = 0.5 * dt
        inverted = []
        for v, vw in enumerate(vws):
            y0 = torch.stack([vw.view(noisy[0])] * 2)
            fn = lambda x, t: model.forward_with_cfg(x, t, pairs[v][0], pairs[v][1], 4.0)
            f0 = fn(y0, torch.full((2,), t0).to("cuda"))
            y_mid = y0 + f0 * half_dt
            noise = -(fn(y_mid, torch.full((2,), t0 + half_dt).to("cuda")) * dt)
            calls += 2
            inverted.append(vw.inverse_view(noise[0]))
        noisy = noisy - torch.stack(inverted).mean(dim=0)
        states.append(noisy[0].clone())
    return torch.stack(states), calls


@pytest.mark.parametrize("name", ["v2", "v3", "v1"])
def test_tiny_trajectories_against_the_reference_batched_and_sequential(golden_dir, name):
    g, cfg, model = _tiny_model(golden_dir)
    vws, caps, mask, z = _tiny_case(g, name)
    V = len(vws)
    grid = [float(v) for v in g["grid"]]
    ref = torch.from_numpy(g[f"{name}_ref"])
    real = {"plain": _bf(g[f"{name}_refbf16"]).float(), "autocast": _bf(g[f"{name}_refbf16ac"]).float(), "choreography": _bf(g[f"{name}_floor"]).float()}
    traj = model.sample_views(z, torch.tensor(grid), vws, caps, mask, "midpoint", cfg_scale=float(g["cfg_scale"]))
    eng = model._engine
    assert traj.shape == ref.shape and eng.last_nfe() == 2 * (len(grid) - 1)  # ONE evaluation of 2 V rows per stage
    _gate(f"views_tiny/{name} batched", traj.float().cpu(), ref, real)
    fin = eng.sample_views(z, torch.tensor(grid), "midpoint", cfg_scale=float(g["cfg_scale"]), return_trajectory=False)
    assert torch.equal(fin[0], traj[-1])
    # the same trajectory one view at a time from Python: V x as many (half-sized) evaluations, same rule
    seq, calls = _sequential(model, vws, caps, mask, z, grid)
    assert calls == 2 * V * (len(grid) - 1)
    _gate(f"views_tiny/{name} sequential", seq.float().cpu(), ref, real)
    print(f"views_tiny/{name}: batched vs sequential, final latent rel-L2 {rel_l2(traj[-1], seq[-1]):.3e}")


def test_batched_path_launches_one_evaluation_per_stage(golden_dir):
    """launch count: a multi-view trajectory of n intervals launches exactly 2 n times the model kernels of ONE forward_with_cfg of 2 V rows
    (the three view kernels are not model kernels and are not counted by the profiling classes)"""
    g, cfg, model = _tiny_model(golden_dir)
    vws, caps, mask, z = _tiny_case(g, "v2")
    grid = torch.tensor([float(v) for v in g["grid"]])
    model.sample_views(z, grid, vws, caps, mask, "midpoint", cfg_scale=4.0)  # warm: engine, prompt, tables
    eng = model._engine

    def launches(fn):
        eng.profile_enable(True)
        eng.profile_reset()
        fn()
        torch.cuda.synchronize()
        n = sum(eng.profile_read(k)[1] for k in range(3))
        eng.profile_enable(False)
        return n

    one = launches(lambda: eng.forward(z.expand(4, -1, -1, -1).contiguous(), torch.full((4,), 0.3), use_cfg=True, cfg_scale=4.0))
    allv = launches(lambda: eng.sample_views(z, grid, "midpoint", cfg_scale=4.0))
    print(f"launches: one forward_with_cfg of 4 rows {one}, a 4-interval midpoint trajectory of 2 views {allv}")
    assert one > 0 and allv == 2 * (len(grid) - 1) * one


def _full_inputs(g, cfg):
    """z and prompts of the full-depth case, regenerated from the seed as scripts/make_views_golden.py drew them (probes in the fixture)"""
    case = json.loads(str(g["case"]))
    rng = np.random.default_rng(case["seed_x"])
    L, lens, neg = case["latent"], case["lens"], int(g["neg_len"])
    z = torch.from_numpy(rng.standard_normal((1, cfg.in_channels, L, L), dtype=np.float32)).to(torch.bfloat16)
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
    assert np.array_equal(z.float().flatten()[:8].numpy(), g["z_probe"]) and np.array_equal(caps.float().flatten()[:8].numpy(), g["caps_probe"])
    return case, z, caps, mask


def test_full_2b_two_views_midpoint_4_intervals_against_the_reference(golden_dir):
    """NextDiT_2B_patch2, all 24 layers, latent 64 x 64 (1024 tokens), views identity + rotate_cw, 4 midpoint intervals with time shift 4:
    against the unmodified reference's loop, model and views in fp32; floor = its own bf16 runs (plain, autocast)"""
    g = np.load(os.path.join(golden_dir, "full_2b_views_mid4.npz"), allow_pickle=False)
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
    case, z, caps, mask = _full_inputs(g, cfg)
    vws = views.get_anagrams_views(case["views"])
    grid = torch.from_numpy(g["grid"])
    traj = model.sample_views(z.cuda(), grid, vws, caps.cuda(), mask.cuda(), "midpoint", cfg_scale=float(g["cfg_scale"]))
    assert model._engine.last_nfe() == 2 * case["intervals"]
    ref = torch.from_numpy(g["ref"])
    _gate("full_2b_views_mid4", traj.float().cpu(), ref, {"plain": _bf(g["refbf16"]).float(), "autocast": _bf(g["refbf16ac"]).float()})
    del model
    torch.cuda.empty_cache()


def test_sample_anagram_end_to_end_with_injected_encoder_and_vae(golden_dir, tmp_path):
    from lumina_t2x_amd import sample_anagram
    g, cfg, model = _tiny_model(golden_dir)

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

    args = sample_anagram.build_parser().parse_args(
        ["--name", "t", "--save_dir", str(tmp_path), "--prompts", "a duck", "a rabbit", "--views", "identity", "rotate_cw", "--style", "a painting of",
         "--num_inference_steps", "4", "--time_shifting_factor", "4", "--cfg_scale", "4", "--seed", "3", "--resolution", "128:128x128"])
    # no checkpoint here: the model is injected, and with it the training resolution the reference reads from model_args.pth
    targs = types.SimpleNamespace(image_size=128, vae="sdxl")
    info = sample_anagram.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode, model=model, train_args=targs)
    assert len(info) == 1 and model._engine.last_nfe() == 2 * 3
    lat = torch.load(info[0]["latent"])
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat.float()).all()
    # what the driver did, by hand
    torch.manual_seed(3)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16)
    feats, mask = sample_anagram.encode_views(encode, ["a duck", "a rabbit"], "a painting of", args.negative_prompt)
    assert feats.shape[0] == 4 and torch.equal(feats[2], feats[3])
    want = model.sample_views(z, sample_anagram.time_grid(4, 4.0), views.get_anagrams_views(["identity", "rotate_cw"]), feats, mask, "midpoint",
                              cfg_scale=4.0, return_trajectory=False)
    assert torch.equal(lat, want.cpu())
    assert os.path.getsize(info[0]["image"]) > 0 and os.path.getsize(info[0]["views_image"]) > 0
    args.upscale = True
    with pytest.raises(NotImplementedError, match="Phase Upscale"):
        sample_anagram.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode, model=model, train_args=targs)
