#!/usr/bin/env python3
"""Tiled (MultiDiffusion) sampling on the 2B Next-DiT with random weights, a 128 x 320 latent canvas (1024 x 2560 pixels) under 128 x 128
windows at stride 64 - 4 windows, a batch of 8 rows, the largest the engine's max_batch of 8 admits -, the CLI's Euler grid, scale 4, on one
box, interleaved, one JSON line:

    tiled      ONE lt_sample_ode_tiled call: per stage a gather, forward_with_cfg of the 8 window rows, a reduce, the canvas combine
    host       the same loop stepped from Python: transport.tiled.sample_tiled around model.forward_with_cfg - per stage the crops, one
               lt_forward_cfg call and fuse in torch (the definition the call is held to, bit for bit)
    whole      a plain lt_sample_ode of the whole canvas as one sample (batch 2: cond + uncond), attention over all 10240 tokens - another
               computation with another result, timed for scale

All are timed ``--rounds`` times after two warm-up runs each, alternating inside a round; reported: ms per step (median, min .. max) and the
ratios.  There is no pass mark.  Random weights: no trained checkpoint is measured and no claim about image quality is made.

    python scripts/bench_tiled.py [--points 10] [--rounds 5] [--small]

Needs a GPU; not part of the test suite.  --small runs a 2-layer model on a 16 x 40 canvas under 16 x 16 windows (a functional check of this
script)."""
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
from lumina_t2x_amd.transport import tiled as T  # noqa: E402
from lumina_t2x_amd.transport.mini import ODE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.device(dev):
        if args.small:
            model = models.NextDiT(dim=576, n_layers=2, n_heads=8, qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
            canvas, win, stride, base = (16, 40), (16, 16), (8, 8), 16
        else:
            model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
            canvas, win, stride, base = (128, 320), (128, 128), (64, 64), (1024 // 16) ** 2
    bench.random_init_(model, seed=0)
    model.eval()
    offs = T.window_grid(*canvas, *win, *stride)
    n = len(offs)
    weight = T.window_weights(*win, "cosine")
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.randn(2 * n, bench.TEXT_LEN, 2048, device=dev, generator=g).to(torch.bfloat16)
    cmask = torch.ones(2 * n, bench.TEXT_LEN, dtype=torch.int32, device=dev)
    cmask[n:, 8:] = 0
    tgrid = ODE(args.points, "euler", 4).t
    steps = len(tgrid) - 1
    z = torch.randn(1, 4, *canvas, device=dev, generator=g).to(torch.bfloat16)
    step_kw = dict(proportional_attn=True, base_seqlen=base, scale_factor=1.0, scale_watershed=1.0)
    kw = dict(cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **step_kw)
    whole_kw = dict(cap_feats=cap[[0, n]].contiguous(), cap_mask=cmask[[0, n]].contiguous(), cfg_scale=4.0, **step_kw)
    z2 = z.repeat(2, 1, 1, 1)
    ways = {
        "whole": lambda: model._engine_sample_ode(z2, tgrid, "euler", True, True, dict(whole_kw)),  # (first: it sizes the engine's max_tokens)
        "tiled": lambda: model.sample_ode_tiled(z, tgrid, (offs, win), cap, cmask, 4.0, method="euler", weights=weight, return_trajectory=True, **step_kw),
        "host": lambda: T.sample_tiled(model.forward_with_cfg, z, tgrid, offs, win, weight, "euler", **kw),
    }
    last, info = {}, {}
    for _ in range(2):  # warm-up: engine, weights, prompt, the graph key of each way (eager use, capture)
        for name, fn in ways.items():
            last[name] = fn()
            torch.cuda.synchronize()
            info[name] = dict(nfe=model._engine.last_nfe(), eval_rows=model._engine.last_eval_rows())
    ms = {k: [] for k in ways}
    for _ in range(args.rounds):
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)

    def stat(vs):
        s = sorted(vs)
        return dict(median=round(s[len(s) // 2], 4), min=round(s[0], 4), max=round(s[-1], 4))

    st = {k: stat(v) for k, v in ms.items()}
    out = {"metric": "tiled_sampling_ms_per_step",
           "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} canvas {canvas[0]}x{canvas[1]} windows {win[0]}x{win[1]} stride {stride[1]} "
                    f"n {n} rows {2 * n} euler {args.points}-point grid scale 4 cosine weights",
           "rounds": args.rounds, "ms_per_step": st,
           "host_over_tiled": round(st["host"]["median"] / st["tiled"]["median"], 5),
           "whole_over_tiled": round(st["whole"]["median"] / st["tiled"]["median"], 5),
           "tiled_spread": round((st["tiled"]["max"] - st["tiled"]["min"]) / st["tiled"]["median"], 5),
           "engine_equals_host_loop": bool(torch.equal(last["tiled"], last["host"])),
           "finite": bool(torch.isfinite(last["tiled"].float()).all()), "calls": info}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
