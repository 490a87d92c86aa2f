#!/usr/bin/env python3
"""Projected guidance (APG, CFG-Zero*) on the 2B Next-DiT with random weights, B = 2, the CLI's 30-point Euler grid, scale 4, at 1024 x 1024 and
256 x 256, on one box, interleaved, one JSON line per resolution:

    schedule   lt_sample_ode_cfg_schedule on a constant table - code this feature does not touch
    apg        lt_sample_ode_cfg_project on the same table, eta 0, momentum -0.5, norm threshold 15: per guided stage one
               guidance_project_stats launch more (it also advances the momentum buffer), and the projected closing kernel
    zero_star  lt_sample_ode_cfg_project, CFG-Zero* without zero-init: the same two launches, no buffer

All three are timed ``--rounds`` times, alternating inside a round; reported: ms per step (median, min .. max), the two ratios to the schedule
call and that call's own spread.  No threshold is set here.  No trained checkpoint is measured and no claim about image quality is made.

    python scripts/bench_project.py [--points 30] [--rounds 5] [--small]

Needs a GPU; not part of the test suite.  --small runs a 2-layer model at 64 x 64 and 32 x 32 latents (a functional check of this script)."""
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
    ap.add_argument("--points", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.device(dev):
        if args.small:
            model = models.NextDiT(dim=576, n_layers=2, n_heads=8, qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
            latents = (64, 32)
        else:
            model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
            latents = (128, 32)
    bench.random_init_(model, seed=0)
    model.eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.randn(2, bench.TEXT_LEN, 2048, device=dev, generator=g).to(torch.bfloat16)
    cmask = torch.ones(2, bench.TEXT_LEN, dtype=torch.int32, device=dev)
    cmask[1, 8:] = 0
    tgrid = ODE(args.points, "euler", 4).t
    n = len(tgrid) - 1
    table = torch.full((n,), 4.0)
    apg = dict(eta=0.0, momentum=-0.5, norm_threshold=15.0)
    for latent in latents:
        z = torch.randn(1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16).repeat(2, 1, 1, 1)
        step_kw = dict(proportional_attn=True, base_seqlen=(1024 // 16) ** 2, scale_factor=1.0, scale_watershed=1.0)

        def run(**kw):
            return model.sample_ode_cfg_schedule(z, tgrid, table, cap, cmask, method="euler", return_trajectory=True, **step_kw, **kw)

        ways = {"schedule": lambda: run(), "apg": lambda: run(apg=apg), "zero_star": lambda: run(zero_star=True)}
        model.forward_with_cfg(z, torch.zeros(2, device=dev), cap, cmask, 4.0, **step_kw)  # engine, weights, prompt
        eng = model._engine
        last, info = {}, {}
        for name, fn in ways.items():  # warm-up: the graph key of each way, twice (eager use, capture)
            fn()
            last[name] = fn()
            torch.cuda.synchronize()
            info[name] = dict(nfe=eng.last_nfe(), eval_rows=eng.last_eval_rows())
        ms = {k: [] for k in ways}
        for _ in range(args.rounds):
            for name, fn in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / n)

        def stat(vs):
            s = sorted(vs)
            return dict(median=round(s[len(s) // 2], 4), min=round(s[0], 4), max=round(s[-1], 4))

        st = {k: stat(v) for k, v in ms.items()}
        out = {"metric": "projected_guidance_ms_per_step",
               "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} latent {latent}x{latent} B2 euler {args.points}-point grid scale 4",
               "apg": apg, "rounds": args.rounds, "ms_per_step": st,
               "apg_over_schedule": round(st["apg"]["median"] / st["schedule"]["median"], 5),
               "zero_star_over_schedule": round(st["zero_star"]["median"] / st["schedule"]["median"], 5),
               "schedule_spread": round((st["schedule"]["max"] - st["schedule"]["min"]) / st["schedule"]["median"], 5),
               "forms_change_the_result": not bool(torch.equal(last["apg"], last["schedule"])) and not bool(torch.equal(last["zero_star"], last["schedule"])),
               "finite": bool(torch.isfinite(last["apg"].float()).all()) and bool(torch.isfinite(last["zero_star"].float()).all()), "calls": info}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
