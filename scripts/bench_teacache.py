#!/usr/bin/env python3
"""Step caching (the TeaCache rule) at the headline shape: the 2B Next-DiT with RANDOM weights, B = 2, guidance scale 4, the euler
grid of the CLI, on one box, the ways alternating inside a round, one JSON line per latent size:

    plain     lt_sample_ode                                   - the existing call, same build: the yardstick (a)
    thr0      lt_sample_ode_cached, threshold 0               - every evaluation runs the stack: the cost of indicator, copy, store and read (b)
    thrX      lt_sample_ode_cached at the thresholds given    - (c)

Reported per way: ms per trajectory (median, min, max), the hit count, lt_last_eval_rows, and the final latent's relative L2 distance from
``plain``.  With RANDOM weights the hit pattern is not a trained model's, and the distances say nothing about image quality.  Derived, not
measured: the added passes of (b) move about 8 M d 2 bytes per evaluation.

    python scripts/bench_teacache.py [--latents 128 32] [--points 11] [--rounds 5] [--thresholds 0.2 0.5 1.0] [--small]

``--latents 128 32`` are 1024^2 and 256^2 images.  Needs a GPU; not part of the test suite.  --small runs a 4-layer model (a functional check
of this script)."""
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
from lumina_t2x_amd.transport.mini import ODE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latents", type=int, nargs="+", default=[128, 32])
    ap.add_argument("--points", type=int, default=11)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.2, 0.5, 1.0])
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.device(dev):
        if args.small:
            model = models.NextDiT(dim=576, n_layers=4, n_heads=8, qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
        else:
            model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
    bench.random_init_(model, seed=0)
    model.eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.randn(2, bench.TEXT_LEN, 2048, device=dev, generator=g).to(torch.bfloat16)
    cmask = torch.ones(2, bench.TEXT_LEN, dtype=torch.int32, device=dev)
    cmask[1, 8:] = 0
    step_kw = dict(proportional_attn=True, base_seqlen=(1024 // 16) ** 2, scale_factor=1.0, scale_watershed=1.0)
    o = ODE(args.points, "euler", 4)
    for latent in args.latents:
        z = torch.randn(1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16).repeat(2, 1, 1, 1)
        ways = {"plain": lambda: o.sample(z, model.forward_with_cfg, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **step_kw)[-1]}
        for thr in [0.0] + list(args.thresholds):
            ways[f"thr{thr:g}"] = (lambda thr=thr: model.sample_ode_teacache(z, o.t, cap, cmask, 4.0, method="euler", threshold=thr, **step_kw))
        info, last = {}, {}
        for name, fn in ways.items():  # warm-up: every graph key of the timed window, twice (eager use, capture)
            fn()
            last[name] = fn()
            torch.cuda.synchronize()
            eng = model._engine
            info[name] = dict(nfe=eng.last_nfe(), eval_rows=eng.last_eval_rows(), hits=0 if name == "plain" else eng.last_cache_hits())
            if name != "plain":
                info[name]["ran"] = "".join(str(int(v)) for v in model.last_cache_stats["stats"][:, 2].tolist())
        ms = {k: [] for k in ways}
        for _ in range(args.rounds):
            for name, fn in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)

        def stat(vs):
            s = sorted(vs)
            return dict(median=round(s[len(s) // 2], 3), min=round(s[0], 3), max=round(s[-1], 3))

        st = {k: stat(v) for k, v in ms.items()}
        plain = last["plain"].float()
        out = {"metric": "teacache_ms_per_trajectory",
               "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} RANDOM weights (the hit pattern is not a trained model's), latent "
                        f"{latent}x{latent} B2 euler {args.points}-point grid, cfg 4",
               "rounds": args.rounds, "ms_per_trajectory": st, "calls": info,
               "thr0_over_plain": round(st["thr0"]["median"] / st["plain"]["median"], 5),
               "plain_spread": round((st["plain"]["max"] - st["plain"]["min"]) / st["plain"]["median"], 5),
               "rel_l2_from_plain": {k: round(float((v.float() - plain).norm() / plain.norm()), 6) for k, v in last.items() if k != "plain"},
               "thr0_final_state_equals_plain": bool(torch.equal(last["thr0"], last["plain"])),
               "added_bytes_per_evaluation_derived": 8 * 2 * (latent // 2) ** 2 * model.dim * 2}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
