"""Phase Upscale (visual-anagram) fixtures: tests/golden/views_upscale_tiny.npz, tests/golden/full_2b_views_upscale_mid2.npz - TEST
INFRASTRUCTURE ONLY.

    python scripts/make_views_upscale_golden.py [tiny] [full]      (authoring container: needs the reference checkout; `full`: ~25 GB RAM)

Drives the guided loop of the reference's visual_anagrams/generate.py:465-494 with the UNMODIFIED pieces: its own `midpoint_solver_extra`
(compiled verbatim from the syntax tree of generate.py, the technique of oracle.ref_harness.load_anagrams_solvers - no source text is copied),
its own view classes and its own model, visual_anagrams/models/nextdit.py, behind oracle/stubs (scripts/make_views_golden.py has the loaders).
The model is built with use_flash_attn=True: in fp32 the module takes its SDPA branch, in bf16 its query-chunked branch over the flash_attn
stand-in.  Nothing under oracle/ is edited.

Per case: ONE latent z (also the `noise` operand), a guidance latent, V views with a prompt each and one negative prompt; over a shifted
4-point grid
  ref        fp32 model, fp32 state
  refbf16    the reference module in bf16 (model.to(bfloat16)), bf16 state        (plain)
  refbf16ac  the same under torch.autocast("cpu", bfloat16), as generate.py:357 wraps the loop
  stage_in / stage_out   model input and output of every stage and view of the refbf16 run (tests walk the chain without a model)
  rest_state / rest_fp32 the loop restated (tests/views_upscale_ref.py: chain_loop) over the same module with the decay factor c rounded to
                         the state dtype / kept in fp32; `c_rounding` records which one equals refbf16 bit for bit
  fwd_*      the first model call of the fp32 run (input, t) with its fp32, bf16 and bf16-autocast outputs: the softmax-rule test's reference
`chunk_gap_*`: what the unmodified bf16 module does on a shape whose query chunks do not reach the last row (the engine refuses it).
"""
import ast
import json
import os
import sys
import time
from functools import partial

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "scripts")]

import make_views_golden as MV  # noqa: E402
import views_upscale_ref as UR  # noqa: E402
from oracle import make_fulldepth_golden as F  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from oracle import synth  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
CFG_SCALE = MV.CFG_SCALE

# name -> (view names, view args, prompt lengths, seed of the views' own random draws, latent (H, W), model kwargs)
TINY_CASES = {
    "up_v2": (["identity", "rotate_cw"], None, [16, 11], 17, (32, 32), dict(proportional_attn=True, base_seqlen=64, scale_factor=2.0)),
    "up_v3": (["flip", "negate", "patch_permute"], [None, None, "4"], [9, 16, 13], 18, (16, 16),
              dict(proportional_attn=False, base_seqlen=None, scale_factor=1.0)),
    "up_v1r": (["flip"], None, [12], 19, (24, 32), dict(proportional_attn=True, base_seqlen=64, scale_factor=1.0)),
    "up_part": (["identity", "flip"], None, [10, 15], 20, (24, 24), dict(proportional_attn=True, base_seqlen=64, scale_factor=1.0)),
}
CHUNK_GAP = dict(latent=(12, 86), base_seqlen=256)  # 258 tokens: int(258 / 256 + 0.99) = 1 chunk of 256 rows


def load_solver_extra():
    """`midpoint_solver_extra` (generate.py:222-262), compiled verbatim from the file's syntax tree into a namespace that holds torch"""
    R.load_anagrams_solvers()  # installs the `.to("cuda")` no-op of the CPU harness
    path = os.path.join(R.REFERENCE_ROOT, "visual_anagrams", "generate.py")
    tree = ast.parse(open(path).read(), filename=path)
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "midpoint_solver_extra"]
    assert len(wanted) == 1 and wanted[0].lineno == 222, [(n.name, n.lineno) for n in wanted]
    ns = {"torch": torch}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), path, "exec"), ns)
    return ns["midpoint_solver_extra"]


def model_kwargs(kw):
    """generate.py:420-435: scale_watershed travels with the call and the fork ignores it"""
    return dict(cfg_scale=CFG_SCALE, proportional_attn=kw["proportional_attn"], base_seqlen=kw["base_seqlen"], scale_factor=kw["scale_factor"],
                scale_watershed=0.3)


def drive(fwd_cfg, views, caps, masks, z, guidance, grid, solver, kw, record=None):
    """generate.py:452-494 with the reference's objects; returns the latent at every grid point [n, C, H, W]"""
    z = z.repeat(2, 1, 1, 1)
    anchor = torch.ones_like(guidance[:1]).to(z.dtype).repeat(2, 1, 1, 1)
    guidance = guidance.repeat(2, 1, 1, 1)
    noisy_img = z.clone()
    states = [noisy_img[0].clone()]

    def recorded(x, t, **k):
        out = fwd_cfg(x, t, **k)
        if record is not None:
            record.append((x[0].clone(), float(t[0]), out[0].clone()))
        return out

    for i in range(len(grid) - 1):
        inverted_noises = []
        for j, view_fn in enumerate(views):
            func = partial(recorded, cap_feats=caps[j], cap_mask=masks[j], **model_kwargs(kw))
            noise = -solver(func, grid[i], grid[i + 1], noisy_img, guidance, z, anchor, view_fn)
            inverted_noises.append(view_fn.inverse_view(noise[0]))
        noisy_img = noisy_img - torch.stack(inverted_noises).mean(dim=0)
        states.append(noisy_img[0].clone())
    return torch.stack(states)


def build_fork(cfg, sd):
    os.environ["TORCHDYNAMO_DISABLE"] = "1"
    mod = F._fresh_import("visual_anagrams", "models.nextdit")
    model = mod.NextDiT(**dict(cfg.ctor_kwargs(), use_flash_attn=True)).eval()
    res = model.load_state_dict(sd, strict=True, assign=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model


def per_view(model, caps, masks, kw):
    """fwd(x [V, C, H, W], t, stage) of tests/views_upscale_ref.py over the module, one view at a time as the reference evaluates it"""
    def fwd(x, t, stage):
        return torch.stack([model.forward_with_cfg(torch.stack([x[v]] * 2), torch.full((2,), t), cap_feats=caps[v], cap_mask=masks[v],
                                                   **model_kwargs(kw))[0] for v in range(x.shape[0])])
    return fwd


def stages(record, V, n):
    """the recorder's (input, t, output) triples, in call order view-major per interval, as [n - 1, 2, V, C, H, W] inputs and outputs"""
    assert len(record) == (n - 1) * V * 2
    xs = torch.stack([r[0] for r in record]).view(n - 1, V, 2, *record[0][0].shape).transpose(1, 2)
    fs = torch.stack([r[2] for r in record]).view(n - 1, V, 2, *record[0][2].shape).transpose(1, 2)
    return xs.contiguous(), fs.contiguous()


def trajectories(cfg, sd, views, pairs, z, guidance, grid, solver, kw, log, tiny):
    out = {}
    caps, masks = [p[0] for p in pairs], [p[1] for p in pairs]
    t0 = time.time()
    model = build_fork(cfg, sd)
    rec32 = []
    out["ref"] = drive(model.forward_with_cfg, views, caps, masks, z, guidance, grid, solver, kw, rec32)
    print(f"[{log}] fp32: {time.time() - t0:.0f} s", flush=True)
    if tiny:  # fp32: the chain is the reference's loop (no rounding points; the two coefficient forms coincide)
        rest = UR.chain_loop(per_view(model, caps, masks, kw), views, z, guidance, z, grid, "fp32")
        err = float((rest - out["ref"]).abs().max())
        assert err < 1e-5, err
    model = model.to(torch.bfloat16)
    capsb = [c.to(torch.bfloat16) for c in caps]
    zb, gb = z.to(torch.bfloat16), guidance.to(torch.bfloat16)
    recb = []
    for ac, key in ((False, "refbf16"), (True, "refbf16ac")):
        t0 = time.time()
        with torch.autocast("cpu", torch.bfloat16, enabled=ac):
            out[key] = drive(model.forward_with_cfg, views, capsb, masks, zb, gb, grid, solver, kw, None if ac else recb)
        assert out[key].dtype == torch.bfloat16
        print(f"[{log}] bf16 {'autocast' if ac else 'plain'}: {time.time() - t0:.0f} s", flush=True)
    if tiny:
        out["stage_in"], out["stage_out"] = stages(recb, len(views), len(grid))
        fwd = per_view(model, capsb, masks, kw)
        eq = {}
        for form in ("state", "fp32"):
            out[f"rest_{form}"] = UR.chain_loop(fwd, views, zb, gb, zb, grid, form)
            eq[form] = torch.equal(out[f"rest_{form}"], out["refbf16"])
        print(f"[{log}] restated bf16 chain equals the reference's bit for bit: c rounded to the state dtype {eq['state']}, c kept fp32 {eq['fp32']}", flush=True)
        assert eq["state"] != eq["fp32"], eq
        out["c_rounding"] = "state" if eq["state"] else "fp32"
        # the first model call of the fp32 run, and the bf16 module on the same input
        x, t, f = rec32[0]
        xin, tt = torch.stack([x] * 2), torch.full((2,), t)
        out["fwd_x"], out["fwd_t"], out["fwd_out"] = x, t, f
        for ac, key in ((False, "fwd_outbf16"), (True, "fwd_outbf16ac")):
            with torch.autocast("cpu", torch.bfloat16, enabled=ac):
                out[key] = model.forward_with_cfg(xin.to(torch.bfloat16), tt, cap_feats=capsb[0], cap_mask=masks[0], **model_kwargs(kw))[0]
    return out


def case_inputs(cfg, seed, lens, hw):
    rng = np.random.default_rng(300 + seed)
    draw = lambda: torch.from_numpy(rng.standard_normal((1, cfg.in_channels) + tuple(hw), dtype=np.float32)).to(torch.bfloat16).float()
    z, guidance = draw(), draw()
    caps, mask, pairs = MV.make_prompts(rng, lens, cfg.cap_feat_dim)
    return z, guidance, caps, mask, pairs


def chunk_gap(cfg, sd):
    """the unmodified bf16 module on a shape whose chunks end before the rows do"""
    H, W = CHUNK_GAP["latent"]
    z, _, _, _, pairs = case_inputs(cfg, 99, [12], (H, W))
    model = build_fork(cfg, sd).to(torch.bfloat16)
    kw = dict(proportional_attn=True, base_seqlen=CHUNK_GAP["base_seqlen"], scale_factor=1.0)
    try:
        out = model.forward_with_cfg(z.repeat(2, 1, 1, 1).to(torch.bfloat16), torch.full((2,), 0.3), cap_feats=pairs[0][0].to(torch.bfloat16),
                                     cap_mask=pairs[0][1], **model_kwargs(kw))
        return f"returned {tuple(out.shape)}, finite: {bool(torch.isfinite(out.float()).all())}"
    except Exception as exc:
        return f"raised {type(exc).__name__}: {str(exc).splitlines()[0][:200]}"


def run_tiny():
    VW = MV.reference_views()
    solver = load_solver_extra()
    cfg = synth.TINY
    sd = synth.synth_state_dict(cfg, seed=0)
    assert MV.pick_model(cfg, sd) == "visual_anagrams"
    grid = MV.time_grid(4, 4.0)
    out = {"config": np.array(json.dumps(cfg.to_dict())), "seed_w": 0, "cfg_scale": CFG_SCALE, "grid": np.array(grid, dtype=np.float32),
           "cases": np.array(json.dumps(list(TINY_CASES))), "neg_len": MV.NEG_LEN}
    rounding = set()
    for name, (vnames, vargs, lens, vseed, hw, kw) in TINY_CASES.items():
        torch.manual_seed(vseed)
        views = VW.get_anagrams_views(vnames, view_args=vargs)
        z, guidance, caps, mask, pairs = case_inputs(cfg, vseed, lens, hw)
        tabs = [MV.view_tables(v, cfg.in_channels, *hw) for v in views]
        tr = trajectories(cfg, sd, views, pairs, z, guidance, grid, solver, kw, f"tiny/{name}", True)
        rounding.add(tr["c_rounding"])
        out.update({f"{name}_views": np.array(json.dumps([vnames, vargs])), f"{name}_view_seed": vseed, f"{name}_lens": np.array(lens),
                    f"{name}_kwargs": np.array(json.dumps(kw)), f"{name}_z": z.numpy(), f"{name}_guidance": guidance.numpy(),
                    f"{name}_caps": MV.bits(caps), f"{name}_mask": mask.numpy(), f"{name}_perm": np.stack([t[0] for t in tabs]),
                    f"{name}_vsign": np.stack([t[2] for t in tabs]), f"{name}_isign": np.stack([t[3] for t in tabs]),
                    f"{name}_ref": tr["ref"].numpy(), f"{name}_fwd_x": tr["fwd_x"].numpy(), f"{name}_fwd_t": np.float32(tr["fwd_t"]),
                    f"{name}_fwd_out": tr["fwd_out"].numpy()})
        for key in ("refbf16", "refbf16ac", "stage_in", "stage_out", "rest_state", "rest_fp32", "fwd_outbf16", "fwd_outbf16ac"):
            out[f"{name}_{key}"] = MV.bits(tr[key])
        print(f"[tiny/{name}] final vs fp32: plain {MV.rel(tr['refbf16'][-1], tr['ref'][-1]):.3e}, autocast "
              f"{MV.rel(tr['refbf16ac'][-1], tr['ref'][-1]):.3e}", flush=True)
    assert len(rounding) == 1, rounding
    out["c_rounding"] = np.array(rounding.pop())
    out["chunk_gap_case"] = np.array(json.dumps(CHUNK_GAP))
    out["chunk_gap_result"] = np.array(chunk_gap(cfg, sd))
    print(f"chunk gap {CHUNK_GAP}: the unmodified module {out['chunk_gap_result']}", flush=True)
    np.savez_compressed(os.path.join(OUT, "views_upscale_tiny.npz"), **out)
    print(f"views_upscale_tiny.npz written; c_rounding = {out['c_rounding']}", flush=True)


FULL = dict(views=["identity", "rotate_cw"], lens=[40, 24], latent=64, seed_w=61, seed_x=262, intervals=2, shift=4.0,
            kwargs=dict(proportional_attn=True, base_seqlen=256, scale_factor=2.0))


def full_inputs(cfg):
    """z, guidance and prompts of the full-depth case from seeds (the fixture stores outputs and probes only)"""
    rng = np.random.default_rng(FULL["seed_x"])
    draw = lambda: torch.from_numpy(rng.standard_normal((1, cfg.in_channels, FULL["latent"], FULL["latent"]), dtype=np.float32)).to(torch.bfloat16).float()
    z, guidance = draw(), draw()
    caps, mask, pairs = MV.make_prompts(rng, FULL["lens"], cfg.cap_feat_dim)
    return z, guidance, caps, mask, pairs


def run_full():
    VW = MV.reference_views()
    solver = load_solver_extra()
    cfg = synth.NEXT_2B
    sd = synth.synth_state_dict(cfg, seed=FULL["seed_w"], streams=True)
    wsum, wprobe, wkeys = F.weight_checksum(sd)
    views = VW.get_anagrams_views(FULL["views"])
    z, guidance, caps, mask, pairs = full_inputs(cfg)
    grid = MV.time_grid(FULL["intervals"] + 1, FULL["shift"])
    tr = trajectories(cfg, sd, views, pairs, z, guidance, grid, solver, FULL["kwargs"], "full_2b_views_upscale_mid2", False)
    out = {"config": np.array(json.dumps(cfg.to_dict())), "cfg_scale": CFG_SCALE, "case": np.array(json.dumps(FULL)), "neg_len": MV.NEG_LEN,
           "wsum": wsum, "wprobe": wprobe, "wkeys": np.array(json.dumps(wkeys)), "grid": np.array(grid, dtype=np.float32),
           "z_probe": z.flatten()[:8].numpy(), "guidance_probe": guidance.flatten()[:8].numpy(), "caps_probe": caps.flatten()[:8].numpy(),
           "ref": tr["ref"].numpy(), "refbf16": MV.bits(tr["refbf16"]), "refbf16ac": MV.bits(tr["refbf16ac"])}
    np.savez_compressed(os.path.join(OUT, "full_2b_views_upscale_mid2.npz"), **out)
    print("full_2b_views_upscale_mid2.npz written; per grid point vs fp32: plain " +
          " ".join(f"{MV.rel(tr['refbf16'][k], tr['ref'][k]):.3e}" for k in range(1, len(grid))) + " | autocast " +
          " ".join(f"{MV.rel(tr['refbf16ac'][k], tr['ref'][k]):.3e}" for k in range(1, len(grid))), flush=True)


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
