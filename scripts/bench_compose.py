#!/usr/bin/env python3
"""Composed guidance on the 2B Next-DiT with RANDOM weights at 1024 x 1024 (a 128 x 128 latent), K = 2 prompts and the base prompt on B' = 1
image - 3 rows per evaluation -, the CLI's Euler grid, weights (4, -1.5), on one box, interleaved, one JSON line:

    compose    ONE lt_sample_ode_compose call: per stage a replicate, a plain forward of the 3 rows, the composition, the state combine
    host       the same loop stepped from Python: transport.guidance.sample_cfg_compose around model.forward - per stage the repeat, one
               lt_forward call and guided_compose in torch (the definition the call is held to, bit for bit)
    floor      a plain lt_sample_ode(use_cfg = 0) of 3 rows on the same grid and conditioning: the evaluations alone, with a 3-row state - the
               floor the composed call is built to sit on (another computation with another result)

All are timed ``--rounds`` times after two warm-up runs each, alternating inside a round; reported: ms per step (median, min .. max) and the
ratios.  There is no pass mark.  Random weights: no trained checkpoint is measured and no claim about image quality is made.

    python scripts/bench_compose.py [--points 10] [--rounds 5] [--small]

Needs a GPU; not part of the test suite.  --small runs a 2-layer model on a 16 x 16 latent (a functional check of this script)."""
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
from lumina_t2x_amd.transport import guidance as G  # noqa: E402
from lumina_t2x_amd.transport.mini import ODE  # noqa: E402

K, BP = 2, 1


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
            hw, base = (16, 16), 16
        else:
            model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
            hw, base = (128, 128), (1024 // 16) ** 2
    bench.random_init_(model, seed=0)
    model.eval()
    rows = (K + 1) * BP
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.randn(rows, bench.TEXT_LEN, 2048, device=dev, generator=g).to(torch.bfloat16)
    cmask = torch.ones(rows, bench.TEXT_LEN, dtype=torch.int32, device=dev)
    cmask[K * BP:, 8:] = 0
    tgrid = ODE(args.points, "euler", 4).t
    steps = len(tgrid) - 1
    table = G.compose_table(tgrid, "euler", [4.0, -1.5])
    z = torch.randn(BP, 4, *hw, device=dev, generator=g).to(torch.bfloat16)
    z3 = z.repeat(K + 1, 1, 1, 1)
    step_kw = dict(proportional_attn=True, base_seqlen=base)
    ways = {
        "compose": lambda: model.sample_ode_compose(z, tgrid, table, cap, cmask, method="euler", return_trajectory=True, **step_kw),
        "host": lambda: G.sample_cfg_compose(model.forward, z, tgrid, table, K, "euler", cap_feats=cap, cap_mask=cmask),
        "floor": lambda: model._engine_sample_ode(z3, tgrid, "euler", False, True, dict(cap_feats=cap, cap_mask=cmask)),
    }
    last, info = {}, {}
    for _ in range(2):  # warm-up: engine, weights, prompt, the one graph key all three ways share (eager use, capture)
        for name, fn in ways.items():
            last[name] = fn()
            torch.cuda.synchronize()
            info[name] = dict(nfe=model._engine.last_nfe(), eval_rows=model._engine.last_eval_rows()) if name != "host" else None
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
    out = {"metric": "composed_guidance_ms_per_step",
           "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} latent {hw[0]}x{hw[1]} K {K} B' {BP} rows {rows} euler {args.points}-point grid "
                    "weights 4 -1.5",
           "rounds": args.rounds, "ms_per_step": st,
           "compose_over_floor": round(st["compose"]["median"] / st["floor"]["median"], 5),
           "host_over_compose": round(st["host"]["median"] / st["compose"]["median"], 5),
           "compose_spread": round((st["compose"]["max"] - st["compose"]["min"]) / st["compose"]["median"], 5),
           "floor_spread": round((st["floor"]["max"] - st["floor"]["min"]) / st["floor"]["median"], 5),
           "engine_equals_host_loop": bool(torch.equal(last["compose"], last["host"])),
           "finite": bool(torch.isfinite(last["compose"].float()).all()), "calls": info}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
