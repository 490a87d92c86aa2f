"""head_dim-128 fixtures (tests/golden/imagenet_tiny_hd128.npz, tests/golden/full_imagenet7b*.npz) - TEST INFRASTRUCTURE ONLY.

    python scripts/make_hd128_golden.py [tiny] [full] [--layers N]      (authoring container: needs the reference checkout, ~62 GB RAM)

Imports oracle.make_golden / oracle.make_fulldepth_golden / oracle.synth / oracle.ref_harness unchanged and adds its own cases:
  imagenet_tiny_hd128   Next-DiT-ImageNet DiT_Llama(dim=256, n_heads=2, n_layers=2, qk_norm=True) on a 16 x 16 latent, the format of
                        imagenet_tiny.npz (oracle.make_golden.family_case writes it)
  full_imagenet7b       DiT_Llama_7B_patch2(qk_norm=True) (dim 4096, 32 heads, 32 layers: head_dim 128), 32 x 32 latent = 256 tokens, the
                        format of full_imagenet600m.npz incl. floor_* / refbf16_* / refbf16ac_*.  With --layers N (a multiple of 8 below
                        32, for a host the full depth does not fit) the file is full_imagenet7b_l<N>.npz and its `config` says so.
What the 7B size changes against oracle.make_fulldepth_golden.run_case: 7.3 B fp32 parameters are 29 GB, so the reference module is built
on the meta device and takes the draw by load_state_dict(assign=True) (no second copy), and the fp32 draw is rounded to bf16 tensor by
tensor (in place of model.to(bfloat16): the same rounding, no fp32 + bf16 set alive together) before the reference's bf16 runs.
"""
import gc
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_fulldepth_golden as F  # noqa: E402
from oracle import make_golden as G  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from oracle import synth  # noqa: E402

TINY_HD128 = synth.NextDiTConfig(dim=256, n_layers=2, n_heads=2, family="imagenet", num_classes=10)


def case_7b(n_layers):
    return dict(cfg=synth.NextDiTConfig(dim=4096, n_layers=n_layers, n_heads=32, family="imagenet"), pkg="Next-DiT-ImageNet",
                module="models.models", cls="DiT_Llama", latent_hw=(32, 32), text_len=0, uncond_len=0, seed_w=131, seed_x=132,
                calls=[("cfg4", 0.5, dict(cfg_scale=4.0))])


def _meta_model(case, sd):
    """the unmodified reference module holding `sd` itself (no copy): parameters created on the meta device, then assigned"""
    os.environ["TORCHDYNAMO_DISABLE"] = "1"
    cfg = case["cfg"]
    mod = F._fresh_import(case["pkg"], case["module"])
    cls = getattr(mod, case["cls"])
    with torch.device("meta"):
        model = cls(**cfg.ctor_kwargs()).eval()
    res = model.load_state_dict(sd, strict=True, assign=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert not any(p.is_meta for p in model.parameters()) and not list(model.buffers())
    # the RoPE table is a plain attribute computed in __init__ (on the meta device above): the module's own function again, on the CPU
    model.freqs_cis = cls.precompute_freqs_cis(cfg.dim // cfg.n_heads, 384)
    return model


def run_full(n_layers):
    name = "full_imagenet7b" if n_layers == 32 else f"full_imagenet7b_l{n_layers}"
    case = case_7b(n_layers)
    F.CASES[name] = case
    cfg = case["cfg"]
    assert cfg.head_dim == 128 and cfg.ffn_hidden == 11008
    t0 = time.time()
    sd = synth.synth_state_dict(cfg, seed=case["seed_w"], streams=True)
    print(f"[{name}] {sum(v.numel() for v in sd.values()) / 1e9:.2f} B parameters drawn in {time.time() - t0:.0f} s", flush=True)
    wsum, wprobe, wkeys = F.weight_checksum(sd)
    tag, tv, ckw = case["calls"][0]

    def inputs():
        ins = list(synth.synth_inputs(cfg, latent_hw=case["latent_hw"], seed=case["seed_x"], t_value=tv))
        ins[0] = ins[0].to(torch.bfloat16).float()  # the engine's inputs are bf16: everyone sees the rounded latent
        return tuple(ins)

    out = {"config": np.array(json.dumps(cfg.to_dict())), "seed_w": case["seed_w"], "seed_x": case["seed_x"],
           "latent_hw": np.array(case["latent_hw"]), "text_len": 0, "uncond_len": 0, "package": np.array(case["pkg"]),
           "wsum": wsum, "wprobe": wprobe, "wkeys": np.array(json.dumps(wkeys)),
           "calls": np.array(json.dumps([[t_, v_, k_] for t_, v_, k_ in case["calls"]])),
           "pinned_by": np.array("reference module output stored as ref_*")}
    rel = lambda a, b: float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
    with torch.no_grad():
        model = _meta_model(case, sd)
        z, t, y = inputs()
        t0 = time.time()
        out[f"ref_{tag}"] = model.forward_with_cfg(z, t, y, ckw["cfg_scale"]).float().numpy().copy()
        print(f"[{name}] reference fp32: {time.time() - t0:.0f} s", flush=True)
        del model
        gc.collect()
        t0 = time.time()
        out[f"oracle_{tag}"] = F.oracle_call(cfg, sd, inputs(), ckw, False).float().numpy()
        t1 = time.time()
        out[f"floor_{tag}"] = F.oracle_call(cfg, sd, inputs(), ckw, True).float().numpy()
        print(f"[{name}] oracle fp32 {t1 - t0:.0f} s, bf16 choreography {time.time() - t1:.0f} s", flush=True)
        print(f"[{name}] oracle vs reference {rel(out[f'oracle_{tag}'], out[f'ref_{tag}']):.3e}; floor vs reference "
              f"{rel(out[f'floor_{tag}'], out[f'ref_{tag}']):.3e}", flush=True)
        np.savez_compressed(os.path.join(F.OUT, f"{name}.npz"), **out)  # (kept if the bf16 leg below runs out of memory)
        for k in list(sd):
            sd[k] = sd[k].to(torch.bfloat16)
        gc.collect()
        model = _meta_model(case, sd)
        for ac, key in ((False, "refbf16"), (True, "refbf16ac")):
            z, t, y = inputs()
            t0 = time.time()
            with torch.autocast("cpu", torch.bfloat16, enabled=ac):
                o = model.forward_with_cfg(z.to(torch.bfloat16), t, y, ckw["cfg_scale"])
            assert o.dtype == torch.bfloat16, o.dtype
            out[f"{key}_{tag}"] = o.float().numpy().copy()
            print(f"[{name}] reference in bf16 ({'autocast' if ac else 'plain'}): {time.time() - t0:.0f} s, vs fp32 reference "
                  f"{rel(out[f'{key}_{tag}'], out[f'ref_{tag}']):.3e} (ch3 {rel(out[f'{key}_{tag}'][:, 3], out[f'ref_{tag}'][:, 3]):.3e})", flush=True)
    fl, base = out[f"floor_{tag}"], out[f"ref_{tag}"]
    print(f"[{name}] floor {rel(fl, base):.3e} (ch3 {rel(fl[:, 3], base[:, 3]):.3e})", flush=True)
    np.savez_compressed(os.path.join(F.OUT, f"{name}.npz"), **out)
    print(f"[{name}] written", flush=True)


def main():
    torch.set_grad_enabled(False)
    assert R.available(), "needs the reference checkout (LUMINA_REFERENCE_ROOT)"
    args = sys.argv[1:]
    layers = 32
    if "--layers" in args:
        layers = int(args[args.index("--layers") + 1])
        assert layers % 8 == 0 and 0 < layers <= 32
    what = [a for a in args if a in ("tiny", "full")] or ["tiny", "full"]
    stubs = os.path.join(REPO, "oracle", "stubs")  # fairscale / flash_attn / torchdiffeq stand-ins the reference modules import
    if stubs not in sys.path:
        sys.path.insert(0, stubs)
    if not torch.cuda.is_available():
        torch.Tensor.cuda = lambda self, *a, **k: self  # the reference hard-codes .cuda() on the label-drop ids
    if "tiny" in what:
        G.family_case("imagenet_tiny_hd128", TINY_HD128, (16, 16), 127, 128)
    if "full" in what:
        run_full(layers)


if __name__ == "__main__":
    main()
