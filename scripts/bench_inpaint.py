#!/usr/bin/env python3
"""Masked (inpainting) sampling at the headline shape (bench.py's cfg2 workload: the 2B Next-DiT, 1024 x 1024, guidance, Euler), three ways on
one box, interleaved, one JSON line:

    plain     lt_sample_ode                       (the unmasked trajectory: what a masked step may not be slower than)
    masked    lt_sample_ode_masked                (the blend inside each step's closing combine)
    stepwise  the same masked trajectory driven per step from Python: forward_with_cfg, the Euler update and the blend as torch ops
              (transport.masked.sample_masked) - what a caller had to do before the engine call existed

    python scripts/bench_inpaint.py [--steps 29] [--warmup 3] [--rounds 3] [--small]

Needs a GPU; not part of the test suite.  --small runs a 2-layer model at a 32 x 32 latent (a functional check of this script)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import bench  # noqa: E402
import lumina_t2x_amd  # noqa: E402,F401
from lumina_t2x_amd import models  # noqa: E402
from lumina_t2x_amd.transport.masked import expand_operands, known, sample_masked  # noqa: E402
from lumina_t2x_amd.transport.mini import ODE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=29)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.device(dev):
        if args.small:
            model = models.NextDiT(dim=576, n_layers=2, n_heads=8, qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
            latent = 32
        else:
            model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
            latent = 128
    bench.random_init_(model, seed=0)
    model.eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.randn(2, bench.TEXT_LEN, 2048, device=dev, generator=g).to(torch.bfloat16)
    cmask = torch.ones(2, bench.TEXT_LEN, dtype=torch.int32, device=dev)
    cmask[1, 8:] = 0
    x1 = torch.randn(1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16)
    noise = torch.randn(1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16)
    mask = torch.zeros(latent, latent, device=dev)
    mask[latent // 4: 3 * latent // 4, latent // 4: 3 * latent // 4] = 1.0
    kw = dict(cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, proportional_attn=True, base_seqlen=(1024 // 16) ** 2, scale_factor=1.0,
              scale_watershed=1.0)

    def grid(nfe):
        return ODE(nfe + 1, "euler", 4).t

    def start(t):
        return known(noise, x1, float(t[0])).repeat(2, 1, 1, 1)

    def plain(nfe):
        t = grid(nfe)
        return model._engine_sample_ode(start(t), t, "euler", True, True, dict(kw))

    def masked(nfe):
        o = ODE(nfe + 1, "euler", 4)
        return o.sample(start(o.t), model.forward_with_cfg, mask=mask, x1=x1, noise=noise, **kw)

    def stepwise(nfe):
        t = grid(nfe)
        z = start(t)
        return sample_masked(model.forward_with_cfg, z, t, *expand_operands(z, mask, x1, noise), "euler", **kw)

    ways = {"plain": plain, "masked": masked, "stepwise": stepwise}
    for fn in ways.values():
        fn(args.warmup)
    torch.cuda.synchronize()
    ms = {k: [] for k in ways}
    last = {}
    for _ in range(args.rounds):
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn(args.steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"metric": "inpaint_ms_per_step", "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} latent {latent}x{latent} B2 cfg euler",
           "steps": args.steps, "rounds": args.rounds, "ms_per_step": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
           "best_ms_per_step": {k: round(min(vs), 4) for k, vs in ms.items()},
           "masked_equals_stepwise": bool(torch.equal(last["masked"], last["stepwise"])),
           "masked_over_plain": round(min(ms["masked"]) / min(ms["plain"]), 5), "stepwise_over_masked": round(min(ms["stepwise"]) / min(ms["masked"]), 5)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
