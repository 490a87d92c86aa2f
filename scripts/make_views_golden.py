"""Multi-view (visual-anagram) fixtures: tests/golden/views_tiny.npz, tests/golden/full_2b_views_mid4.npz - TEST INFRASTRUCTURE ONLY.

    python scripts/make_views_golden.py [tiny] [full]        (authoring container: needs the reference checkout; `full`: ~20 GB RAM)

Drives Phase Init of the reference's visual_anagrams/generate.py:389-414 with the UNMODIFIED pieces: its own `midpoint_solver`
(oracle.ref_harness.load_anagrams_solvers), its own view classes (visual_anagrams/visual_anagrams/views, imported behind an empty
stand-in for `torchvision`, which only make_frame and out-of-scope views use) and its own model (visual_anagrams/models/nextdit.py behind
oracle/stubs; the script asserts that it equals lumina_next_t2i's NextDiT in fp32 on the tiny config).  Nothing under oracle/ is edited.

Per case: ONE latent z, V views with a prompt each (different lengths) and one negative prompt; the trajectory over a shifted 5-point grid
  ref        fp32 model, fp32 state
  refbf16    the reference module in bf16 (model.to(bfloat16)), bf16 state        (plain)
  refbf16ac  the same under torch.autocast("cpu", bfloat16), as generate.py:357 wraps the loop
  floor      (tiny only) the loop restated here over the bf16-choreography oracle (oracle.nextdit_oracle, bf16=True)
`dt_rounding`: dt / half_dt are Python floats in generate.py:212-219.  The bf16 trajectory is restated here twice over the reference module
- scalar kept in fp32 for the multiply vs cast to bf16 first - and the one that equals refbf16 bit for bit is recorded; the engine follows it.
View tables (`vt_*`): for every built view name, perm / iperm / vsign / isign extracted from the reference class by pushing an index image
and a ones image through view() / inverse_view(), plus its outputs on a random tensor (tests/test_views_cpu.py compares without the
reference).
"""
import importlib
import json
import os
import sys
import time
import types
from functools import partial

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_fulldepth_golden as F  # noqa: E402
from oracle import nextdit_oracle as O  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from oracle import synth  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
CFG_SCALE = 4.0
NEG_LEN = 8

# name -> (view names, view args, prompt lengths, seed of the views' own random draws)
TINY_CASES = {
    "v2": (["identity", "rotate_cw"], None, [16, 11], 7),
    "v3": (["flip", "negate", "patch_permute"], [None, None, "4"], [9, 16, 13], 8),
    "v1": (["rotate_180"], None, [12], 9),
}
# view tables for the CPU test: name -> (arg, H = W)
TABLE_VIEWS = {"identity": (None, 16), "flip": (None, 16), "rotate_cw": (None, 16), "rotate_ccw": (None, 16), "rotate_180": (None, 16),
               "negate": (None, 16), "patch_permute": ("4", 16), "pixel_permute": (None, 64)}


class _Standin(types.ModuleType):
    """an EMPTY module standing in for torchvision (absent here): attribute access yields further stand-ins, nothing is callable"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        m = _Standin(f"{self.__name__}.{name}")
        setattr(self, name, m)
        return m


def reference_views():
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
        if name not in sys.modules:
            sys.modules[name] = _Standin(name)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    root = os.path.join(R.REFERENCE_ROOT, "visual_anagrams")
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module("visual_anagrams.views")


def view_tables(view, C, H, W):
    """(perm, iperm, vsign, isign) of a reference view object, read off its own view() / inverse_view()"""
    idx = torch.arange(H * W, dtype=torch.float32).view(1, H, W).repeat(C, 1, 1)
    ones = torch.ones(C, H, W)
    sv, si = view.view(ones), view.inverse_view(ones)
    perm = (view.view(idx) * sv)[0].flatten().round().to(torch.int32)
    iperm = (view.inverse_view(idx) * si)[0].flatten().round().to(torch.int32)
    return perm.numpy(), iperm.numpy(), sv[:, 0, 0].numpy().copy(), si[:, 0, 0].numpy().copy()


def time_grid(n, shift):
    t = torch.linspace(0.0, 1.0, n)  # generate.py:378-385
    if shift:
        t = t / (t + shift - shift * t)
    return t.tolist()


def drive(fwd_cfg, views, caps, masks, z, grid, solver):
    """generate.py:389-414 with the reference's objects; returns the latent at every grid point [n, C, H, W]"""
    noisy_img = z.repeat(2, 1, 1, 1)
    states = [noisy_img[0].clone()]
    for i in range(len(grid) - 1):
        inverted_noises = []
        for j, view_fn in enumerate(views):
            viewed = torch.stack([view_fn.view(noisy_img[0])] * 2)
            func = partial(fwd_cfg, cap_feats=caps[j], cap_mask=masks[j], cfg_scale=CFG_SCALE)
            noise = -solver(func, grid[i], grid[i + 1], viewed)
            inverted_noises.append(view_fn.inverse_view(noise[0]))
        noisy_img = noisy_img - torch.stack(inverted_noises).mean(dim=0)
        states.append(noisy_img[0].clone())
    return torch.stack(states)


def restated(fwd_cfg, views, caps, masks, z, grid, scalar_dtype):
    """the same loop written out, with the scalar of `tensor * python_float` cast to `scalar_dtype` before the multiply"""
    y = z[0].clone()
    states = [y.clone()]
    sc = lambda v: torch.tensor(v, dtype=torch.float32).to(scalar_dtype).float()
    mul = lambda a, v: (a.float() * sc(v)).to(a.dtype)
    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = t1 - t0
        half_dt = 0.5 * dt
        acc = []
        for j, vw in enumerate(views):
            x = torch.stack([vw.view(y)] * 2)
            f0 = fwd_cfg(x, torch.full((2,), t0), cap_feats=caps[j], cap_mask=masks[j], cfg_scale=CFG_SCALE)
            xm = x + mul(f0, half_dt)
            f1 = fwd_cfg(xm, torch.full((2,), t0 + half_dt), cap_feats=caps[j], cap_mask=masks[j], cfg_scale=CFG_SCALE)
            acc.append(vw.inverse_view(-mul(f1, dt)[0]))
        y = y - torch.stack(acc).mean(dim=0)
        states.append(y.clone())
    return torch.stack(states)


def make_prompts(rng, lens, cap_dim):
    """engine layout: rows 0..V-1 the view prompts, rows V..2V-1 the negative prompt; T = longest, rounded up to 8.  Returns the
    [2V, T, D] / [2V, T] arrays and the per-view (prompt, negative) pairs cut to that pair's own padded length (generate.py:344-351)"""
    V = len(lens)
    T = (max(lens + [NEG_LEN]) + 7) // 8 * 8
    caps = torch.zeros(2 * V, T, cap_dim)
    mask = torch.zeros(2 * V, T, dtype=torch.int32)
    neg = torch.from_numpy(rng.standard_normal((NEG_LEN, cap_dim), dtype=np.float32))
    for v, n in enumerate(lens):
        caps[v, :n] = torch.from_numpy(rng.standard_normal((n, cap_dim), dtype=np.float32))
        mask[v, :n] = 1
        caps[V + v, :NEG_LEN] = neg
        mask[V + v, :NEG_LEN] = 1
    # padding positions carry arbitrary (masked) features, as a text encoder's output does
    pad = torch.from_numpy(rng.standard_normal((2 * V, T, cap_dim), dtype=np.float32))
    caps = torch.where(mask.bool().unsqueeze(-1), caps, pad).to(torch.bfloat16).float()
    pairs = []
    for v, n in enumerate(lens):
        Tv = (max(n, NEG_LEN) + 7) // 8 * 8
        pairs.append((caps[[v, V + v], :Tv].clone(), mask[[v, V + v], :Tv].clone()))
    return caps, mask, pairs


def build_model(cfg, sd, which):
    os.environ["TORCHDYNAMO_DISABLE"] = "1"
    pkg, module = ("visual_anagrams", "models.nextdit") if which == "visual_anagrams" else ("lumina_next_t2i", "models.model")
    mod = F._fresh_import(pkg, module)
    kw = cfg.ctor_kwargs()
    if "use_flash_attn" in mod.NextDiT.__init__.__code__.co_varnames:
        kw["use_flash_attn"] = False
    model = mod.NextDiT(**kw).eval()
    res = model.load_state_dict(sd, strict=True, assign=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model


def pick_model(cfg, sd):
    """the anagram fork where it imports and equals lumina_next_t2i's NextDiT in fp32 on the tiny config; records which"""
    z, t, cap, mask = synth.synth_inputs(cfg)
    base = build_model(cfg, sd, "lumina_next_t2i").forward_with_cfg(z, t, cap, mask, CFG_SCALE)
    try:
        fork = build_model(cfg, sd, "visual_anagrams")
    except Exception as exc:  # does not import behind the stubs
        print(f"visual_anagrams/models/nextdit.py does not import here ({type(exc).__name__}: {exc}); using lumina_next_t2i", flush=True)
        return "lumina_next_t2i"
    out = fork.forward_with_cfg(z, t, cap, mask, CFG_SCALE)
    assert torch.equal(out, base), f"the anagram fork differs from lumina_next_t2i in fp32: max abs {float((out - base).abs().max()):.3e}"
    return "visual_anagrams"


def trajectories(cfg, sd, which, views, pairs, z, grid, solver, floor, log):
    out = {}
    caps = [p[0] for p in pairs]
    masks = [p[1] for p in pairs]
    t0 = time.time()
    model = build_model(cfg, sd, which)
    out["ref"] = drive(model.forward_with_cfg, views, caps, masks, z, grid, solver)
    print(f"[{log}] fp32: {time.time() - t0:.0f} s", flush=True)
    model = model.to(torch.bfloat16)
    capsb = [c.to(torch.bfloat16) for c in caps]
    zb = z.to(torch.bfloat16)
    for ac, key in ((False, "refbf16"), (True, "refbf16ac")):
        t0 = time.time()
        with torch.autocast("cpu", torch.bfloat16, enabled=ac):
            out[key] = drive(model.forward_with_cfg, views, capsb, masks, zb, grid, solver)
        assert out[key].dtype == torch.bfloat16
        print(f"[{log}] bf16 {'autocast' if ac else 'plain'}: {time.time() - t0:.0f} s", flush=True)
    if floor:
        orc = lambda x, t, cap_feats, cap_mask, cfg_scale: O.forward_with_cfg(sd, cfg, x.float(), t, cap_feats.float(), cap_mask, cfg_scale,
                                                                              bf16=True).to(x.dtype)
        # fp32 restatement against the reference loop first: the restated loop is the reference's
        fl32 = restated(lambda x, t, cap_feats, cap_mask, cfg_scale: O.forward_with_cfg(sd, cfg, x, t, cap_feats, cap_mask, cfg_scale), views, caps,
                        masks, z, grid, torch.float32)
        err = float((fl32 - out["ref"]).abs().max())
        assert err < 1e-4, err
        eq = {}
        for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            eq[name] = torch.equal(restated(model.forward_with_cfg, views, capsb, masks, zb, grid, dt), out["refbf16"])
        print(f"[{log}] restated bf16 loop equals the reference's bit for bit: scalar kept fp32 {eq['fp32']}, scalar cast to bf16 {eq['bf16']}", flush=True)
        assert eq["fp32"] != eq["bf16"], eq
        out["dt_rounding"] = "fp32" if eq["fp32"] else "bf16"
        out["floor"] = restated(orc, views, capsb, masks, zb, grid, torch.float32 if eq["fp32"] else torch.bfloat16)
    return out


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def bits(x):
    return x.to(torch.bfloat16).view(torch.int16).numpy().copy()


def run_tiny():
    VW = reference_views()
    solver = R.load_anagrams_solvers()
    cfg = synth.TINY
    sd = synth.synth_state_dict(cfg, seed=0)
    which = pick_model(cfg, sd)
    print(f"model: {which}", flush=True)
    H = W = 16
    grid = time_grid(5, 4.0)
    out = {"config": np.array(json.dumps(cfg.to_dict())), "seed_w": 0, "model": np.array(which), "cfg_scale": CFG_SCALE,
           "grid": np.array(grid, dtype=np.float32), "cases": np.array(json.dumps(list(TINY_CASES))), "neg_len": NEG_LEN}
    rounding = set()
    for name, (vnames, vargs, lens, vseed) in TINY_CASES.items():
        torch.manual_seed(vseed)
        views = VW.get_anagrams_views(vnames, view_args=vargs)
        rng = np.random.default_rng(100 + vseed)
        z = torch.from_numpy(rng.standard_normal((1, cfg.in_channels, H, W), dtype=np.float32)).to(torch.bfloat16).float()
        caps, mask, pairs = make_prompts(rng, lens, cfg.cap_feat_dim)
        tabs = [view_tables(v, cfg.in_channels, H, W) for v in views]
        tr = trajectories(cfg, sd, which, views, pairs, z, grid, solver, True, f"tiny/{name}")
        rounding.add(tr["dt_rounding"])
        out.update({f"{name}_views": np.array(json.dumps([vnames, vargs])), f"{name}_view_seed": vseed, f"{name}_lens": np.array(lens),
                    f"{name}_z": z.numpy(), f"{name}_caps": bits(caps), f"{name}_mask": mask.numpy(),
                    f"{name}_perm": np.stack([t[0] for t in tabs]), f"{name}_vsign": np.stack([t[2] for t in tabs]),
                    f"{name}_isign": np.stack([t[3] for t in tabs]), f"{name}_ref": tr["ref"].numpy(), f"{name}_refbf16": bits(tr["refbf16"]),
                    f"{name}_refbf16ac": bits(tr["refbf16ac"]), f"{name}_floor": bits(tr["floor"])})
        print(f"[tiny/{name}] final vs fp32: plain {rel(tr['refbf16'][-1], tr['ref'][-1]):.3e}, autocast {rel(tr['refbf16ac'][-1], tr['ref'][-1]):.3e}, "
              f"choreography {rel(tr['floor'][-1], tr['ref'][-1]):.3e}", flush=True)
    assert len(rounding) == 1, rounding
    out["dt_rounding"] = np.array(rounding.pop())
    # view tables + outputs on a random tensor, per built view name
    g = torch.Generator().manual_seed(5)
    for vname, (arg, hw) in TABLE_VIEWS.items():
        torch.manual_seed(11)
        view = VW.get_anagrams_views([vname], view_args=[arg])[0]
        perm, iperm, vs, isg = view_tables(view, 4, hw, hw)
        x = torch.randn(4, hw, hw, generator=g)
        out.update({f"vt_{vname}_perm": perm, f"vt_{vname}_iperm": iperm, f"vt_{vname}_vsign": vs, f"vt_{vname}_isign": isg,
                    f"vt_{vname}_x": x.numpy(), f"vt_{vname}_view": view.view(x).numpy().copy(),
                    f"vt_{vname}_inv": view.inverse_view(x).numpy().copy()})
    out["vt_names"] = np.array(json.dumps({k: [a, hw] for k, (a, hw) in TABLE_VIEWS.items()}))
    out["vt_seed"] = 11
    np.savez_compressed(os.path.join(OUT, "views_tiny.npz"), **out)
    print(f"views_tiny.npz written; dt_rounding = {out['dt_rounding']}", flush=True)


FULL = dict(views=["identity", "rotate_cw"], lens=[40, 24], latent=64, seed_w=61, seed_x=162, intervals=4, shift=4.0)


def full_inputs(cfg):
    """z and prompts of the full-depth case from seeds (the fixture stores outputs only; tests/test_gpu_views.py calls this too)"""
    rng = np.random.default_rng(FULL["seed_x"])
    z = torch.from_numpy(rng.standard_normal((1, cfg.in_channels, FULL["latent"], FULL["latent"]), dtype=np.float32)).to(torch.bfloat16).float()
    caps, mask, pairs = make_prompts(rng, FULL["lens"], cfg.cap_feat_dim)
    return z, caps, mask, pairs


def run_full():
    VW = reference_views()
    solver = R.load_anagrams_solvers()
    cfg = synth.NEXT_2B
    tiny_sd = synth.synth_state_dict(synth.TINY, seed=0)
    which = pick_model(synth.TINY, tiny_sd)
    sd = synth.synth_state_dict(cfg, seed=FULL["seed_w"], streams=True)
    wsum, wprobe, wkeys = F.weight_checksum(sd)
    views = VW.get_anagrams_views(FULL["views"])
    z, caps, mask, pairs = full_inputs(cfg)
    grid = time_grid(FULL["intervals"] + 1, FULL["shift"])
    tr = trajectories(cfg, sd, which, views, pairs, z, grid, solver, False, "full_2b_views_mid4")
    out = {"config": np.array(json.dumps(cfg.to_dict())), "model": np.array(which), "cfg_scale": CFG_SCALE, "case": np.array(json.dumps(FULL)),
           "neg_len": NEG_LEN, "wsum": wsum, "wprobe": wprobe, "wkeys": np.array(json.dumps(wkeys)), "grid": np.array(grid, dtype=np.float32),
           "z_probe": z.flatten()[:8].numpy(), "caps_probe": caps.flatten()[:8].numpy(),
           "ref": tr["ref"].numpy(), "refbf16": bits(tr["refbf16"]), "refbf16ac": bits(tr["refbf16ac"])}
    np.savez_compressed(os.path.join(OUT, "full_2b_views_mid4.npz"), **out)
    print("full_2b_views_mid4.npz written; per grid point vs fp32: plain " + " ".join(f"{rel(tr['refbf16'][k], tr['ref'][k]):.3e}" for k in range(1, len(grid))) +
          " | autocast " + " ".join(f"{rel(tr['refbf16ac'][k], tr['ref'][k]):.3e}" for k in range(1, len(grid))), flush=True)


def main():
    torch.set_grad_enabled(False)
    assert R.available(), "needs the reference checkout (LUMINA_REFERENCE_ROOT)"
    what = [a for a in sys.argv[1:] if a in ("tiny", "full")] or ["tiny", "full"]
    if "tiny" in what:
        run_tiny()
    if "full" in what:
        run_full()


if __name__ == "__main__":
    main()
