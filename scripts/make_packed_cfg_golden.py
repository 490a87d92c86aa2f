"""Guidance on a size list: tests/golden/nextdit_tiny_packed_cfg.npz - TEST INFRASTRUCTURE ONLY.

    python scripts/make_packed_cfg_golden.py        (authoring container: needs the reference checkout)

The reference's forward_with_cfg takes tensors only (lumina_next_t2i/models/model.py:901-902), so the list form is a composition of two
UNMODIFIED pieces: NextDiT.forward on the list [x_0 .. x_{B'-1}, x_0 .. x_{B'-1}] (the list branch, model.py:789-834, CPU fp32 - the SDPA
branch with the key mask) and the three-line guidance expression of model.py:908-911, applied here per sample on the first three channels
(the `cfg_channels` quirk); the remaining channels are each row's own.  Nothing under oracle/ is edited.

Case: the tiny config, three images (2 B' = 6 rows) at latents 12x20, 16x16 and 6x16 = 60, 64 and 24 tokens - two non-square, the longest
not first, one count no multiple of 64, one under half a tile, three widths; captions of different lengths; plain attention and
proportional attention with base_seqlen 16 (as forward_with_cfg leaves the flags on the layers, model.py:891-899; the scale sees the padded
length, :373-374).  Per-evaluation outputs only: the reference has no list sampler to record.
  fwd{b} / fwdprop{b}    the list forward's output of row b (2 B' rows)
  cfg{b} / cfgprop{b}    after guidance at CFG_SCALE
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import ref_harness as R  # noqa: E402
from oracle import synth  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
CFG_SCALE = 4.0
SIZES = [(12, 20), (16, 16), (6, 16)]
TEXT_LEN = 16
SEED_W, SEED_X = 21, 22


def guide(outs, scale):
    """model.py:908-913 per sample: eps = out[:3], half_eps = uncond + scale * (cond - uncond) on both rows, the rest untouched"""
    half = len(outs) // 2
    res = []
    for b, y in enumerate(outs):
        cond_eps, uncond_eps = outs[b % half][:3], outs[b % half + half][:3]
        half_eps = uncond_eps + scale * (cond_eps - uncond_eps)
        res.append(torch.cat([half_eps, y[3:]], dim=0))
    return res


def main():
    cfg = synth.TINY
    sd = synth.synth_state_dict(cfg, seed=SEED_W)
    R.load_reference("lumina_next_t2i")
    model = R.build_reference_model(cfg, sd)
    rng = np.random.default_rng(SEED_X)
    half = len(SIZES)
    B = 2 * half
    xs = [torch.from_numpy(rng.standard_normal((cfg.in_channels, h, w), dtype=np.float32)) for h, w in SIZES]
    t1 = rng.uniform(0.1, 0.9, size=half).astype(np.float32)
    t = torch.from_numpy(np.concatenate([t1, t1]))
    cap = torch.from_numpy(rng.standard_normal((B, TEXT_LEN, cfg.cap_feat_dim), dtype=np.float32))
    mask = torch.ones(B, TEXT_LEN, dtype=torch.int32)
    for b in range(half):
        mask[b, TEXT_LEN - 2 * b:] = 0      # cond prompts of 16, 14, 12 tokens
        mask[half + b, 6 - b:] = 0          # negative prompts of 6, 5, 4 tokens
    out = {"config": np.array(json.dumps(cfg.to_dict())), "seed_w": SEED_W, "seed_x": SEED_X, "sizes": np.array(SIZES, dtype=np.int32),
           "cfg_scale": np.float32(CFG_SCALE), "t": t.numpy(), "cap": cap.numpy(), "mask": mask.numpy()}
    for b, x in enumerate(xs):
        out[f"x{b}"] = x.numpy()
    with torch.no_grad():
        for key, prop in (("", False), ("prop", True)):
            for layer in model.layers:  # model.py:891-899
                layer.attention.proportional_attn, layer.attention.base_seqlen = prop, (16 if prop else None)
            ys = model(xs + xs, t, cap, mask)
            assert isinstance(ys, list) and all(tuple(y.shape) == (cfg.in_channels,) + SIZES[b % half] for b, y in enumerate(ys))
            for b, (y, g) in enumerate(zip(ys, guide(ys, CFG_SCALE))):
                out[f"fwd{key}{b}"], out[f"cfg{key}{b}"] = y.numpy(), g.numpy()
    path = os.path.join(OUT, "nextdit_tiny_packed_cfg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", SIZES)


if __name__ == "__main__":
    main()
