#!/usr/bin/env python3
"""Guidance reuse at the headline shape (the 2B Next-DiT with RANDOM weights, 1024 x 1024, B = 2, scale 4), euler and midpoint, on one box,
interleaved, one JSON line per method:

    full       lt_sample_ode_cfg_schedule, every entry 4       - the existing call, same build: the yardstick
    every2/3   lt_sample_ode_cfg_reuse, a refresh on every 2nd / 3rd guided evaluation, the cond row alone in between
    per_step   (midpoint) a refresh on the first stage of each step, a reuse on the second
    floor2/3   lt_sample_ode_cfg_schedule on a table with the SAME number of half-row stages in the same places, run as conditional-only
               stages (scale 1): what the half-row evaluations cost without the closing kernel's read of the difference

Every way is timed ``--rounds`` times, the ways alternating inside a round.  Reported per way: ms per trajectory (median, min, max),
``lt_last_eval_rows``, the ``layout_flips`` option of the call (conversions of all GEMM weights between the row-major and the pair layout,
which happen when the 2 B'- and the B'-row evaluations straddle the pair-layout threshold) and ``last_pair``; the relative L2 of each final
latent from the full-guidance one; the ratio of each reuse way to its floor, and the cost of one reuse stage over one conditional-only stage
derived from it.  Random weights: the distances say how far the trajectories lie apart on THIS model, nothing about image quality.

    python scripts/bench_guidance_reuse.py [--latent 128] [--points 30] [--rounds 5] [--methods euler midpoint] [--small]

``--latent 32`` is the 512-row configuration (2 x 256 tokens; the reuse stages run 256 rows).  Needs a GPU; not part of the test suite.
--small runs a 2-layer model (a functional check of this script)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--points", type=int, default=30, help="grid points of the euler run; midpoint runs (points + 1) // 2 + 1 for the same NFE")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--methods", nargs="+", default=["euler", "midpoint"])
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.device(dev):
        if args.small:
            model = models.NextDiT(dim=576, n_layers=2, n_heads=8, qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
        else:
            model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
    latent = args.latent
    bench.random_init_(model, seed=0)
    model.eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.randn(2, bench.TEXT_LEN, 2048, device=dev, generator=g).to(torch.bfloat16)
    cmask = torch.ones(2, bench.TEXT_LEN, dtype=torch.int32, device=dev)
    cmask[1, 8:] = 0
    z = torch.randn(1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16).repeat(2, 1, 1, 1)
    step_kw = dict(proportional_attn=True, base_seqlen=(1024 // 16) ** 2, scale_factor=1.0, scale_watershed=1.0)
    model.forward_with_cfg(z, torch.zeros(2, device=dev), cap, cmask, 4.0, **step_kw)  # engine, weights, the flags a plain forward reads
    eng = model._engine

    for method in args.methods:
        points = args.points if method == "euler" else (args.points + 1) // 2 + 1
        tgrid = ODE(points, method, 4).t
        stages = 1 if method == "euler" else 2
        n = (len(tgrid) - 1) * stages
        fours = torch.full((n,), 4.0)
        flags = {"every2": G.cfg_reuse_table(tgrid, method, fours, every=2), "every3": G.cfg_reuse_table(tgrid, method, fours, every=3)}
        if method == "midpoint":
            flags["per_step"] = G.cfg_reuse_table(tgrid, method, fours, per_step=True)

        def schedule(table):
            return lambda: model.sample_ode_cfg_schedule(z, tgrid, table, cap, cmask, method=method, **step_kw)

        def reuse(f):
            return lambda: model.sample_ode_cfg_schedule(z, tgrid, fours, cap, cmask, method=method, reuse=f, **step_kw)

        ways = {"full": schedule(fours)}
        for name, f in flags.items():
            ways[name] = reuse(f)
            ways["floor_" + name] = schedule(torch.where(f == 1, torch.tensor(1.0), fours))  # the same stages, conditional-only
        info, last = {}, {}
        for name, fn in ways.items():  # warm-up: every shape and graph key of the timed window, twice (eager use, capture)
            fn()
            last[name] = fn()
            torch.cuda.synchronize()
            info[name] = dict(nfe=eng.last_nfe(), eval_rows=eng.last_eval_rows(), layout_flips=eng.get_option("layout_flips"),
                              last_pair=eng.get_option("last_pair"))
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
        full = last["full"].float()
        rel = {k: round(float((v.float() - full).norm() / full.norm()), 6) for k, v in last.items()}
        t_full = st["full"]["median"] / n  # one 2 B'-row evaluation
        ratios = {}
        for name, f in flags.items():
            r = int(f.sum())
            over = st[name]["median"] / st["floor_" + name]["median"]
            # (floor - refresh stages) / r is one conditional-only stage; the reuse way's excess over the floor, spread over its r reuse stages
            t_cond = (st["floor_" + name]["median"] - (n - r) * t_full) / r
            t_reuse = (st[name]["median"] - (n - r) * t_full) / r
            ratios[name] = dict(reuse_stages=r, over_floor=round(over, 5), over_full=round(st[name]["median"] / st["full"]["median"], 5),
                                ms_cond_only_stage=round(t_cond, 4), ms_reuse_stage=round(t_reuse, 4), reuse_over_cond_only=round(t_reuse / t_cond, 5))
        out = {"metric": "guidance_reuse_ms_per_trajectory",
               "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} random weights, latent {latent}x{latent} B2 {method} {points}-point grid "
                        f"({n} evaluations) scale 4",
               "rows_per_evaluation": {"refresh": 2 * (latent // 2) ** 2, "reuse": (latent // 2) ** 2},
               "rounds": args.rounds, "ms_per_trajectory": st, "ms_per_full_evaluation": round(t_full, 4), "calls": info, "reuse": ratios,
               "rel_l2_from_full_guidance": rel,
               "full_spread": round((st["full"]["max"] - st["full"]["min"]) / st["full"]["median"], 5)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
