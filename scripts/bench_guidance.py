#!/usr/bin/env python3
"""Guidance schedules at the headline shape (bench.py's cfg2 workload: the 2B Next-DiT, 1024 x 1024, B = 2, a 30-point Euler grid, scale 4),
on one box, interleaved, one JSON line:

    ode        (a) lt_sample_ode at scale 4                    - code this feature does not touch: the trajectory as it was
    constant   (b) lt_sample_ode_cfg_schedule, all entries 4   - the same evaluations, the scale read from device memory
    keep100/60/30  (c) intervals that leave 100 % / 60 % / 30 % of the stages guided; the others evaluate the cond row alone
    host60/30  (d) the interval trajectories stepped from Python (transport.guidance.sample_cfg_schedule)
    T_B, T_Bh  per-evaluation time of the B-row guided and the B'-row conditional trajectory (all-4 and all-1 tables)

Every way is timed ``--rounds`` times, the ways alternating inside a round; a figure is reported with its spread over the rounds.  The floor of
an interval trajectory with G guided and C conditional stages is G * T_B + C * T_Bh.  Also reported: the weight layout each regime runs on
(``last_pair``) and the layout conversions of each interval call (``layout_flips``).

    python scripts/bench_guidance.py [--points 30] [--rounds 5] [--small] [--no-host]

Needs a GPU; not part of the test suite.  --small runs a 2-layer model at a 64 x 64 latent (a functional check of this script)."""
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


def keep_table(tgrid, frac, scale=4.0):
    """guidance on the first ``frac`` of the Euler stages (the noisy end), scale 1 on the rest"""
    n = len(tgrid) - 1
    g = int(round(frac * n))
    return torch.tensor([scale] * g + [1.0] * (n - g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip (d), the Python-stepped trajectories")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.device(dev):
        if args.small:
            model = models.NextDiT(dim=576, n_layers=2, n_heads=8, qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
            latent = 64
        else:
            model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=2048).to(torch.bfloat16)
            latent = 128
    bench.random_init_(model, seed=0)
    model.eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.randn(2, bench.TEXT_LEN, 2048, device=dev, generator=g).to(torch.bfloat16)
    cmask = torch.ones(2, bench.TEXT_LEN, dtype=torch.int32, device=dev)
    cmask[1, 8:] = 0
    z = torch.randn(1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16).repeat(2, 1, 1, 1)
    step_kw = dict(proportional_attn=True, base_seqlen=(1024 // 16) ** 2, scale_factor=1.0, scale_watershed=1.0)
    tgrid = ODE(args.points, "euler", 4).t
    n = len(tgrid) - 1
    tables = {"constant": keep_table(tgrid, 1.0), "keep100": keep_table(tgrid, 1.0), "keep60": keep_table(tgrid, 0.6), "keep30": keep_table(tgrid, 0.3),
              "T_Bh": keep_table(tgrid, 0.0)}

    def ode():
        return model._engine_sample_ode(z, tgrid, "euler", True, True, dict(cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **step_kw))

    def engine(name):
        return lambda: model.sample_ode_cfg_schedule(z, tgrid, tables[name], cap, cmask, method="euler", return_trajectory=True, **step_kw)

    def host(name):
        return lambda: G.sample_cfg_schedule(model, z, tgrid, tables[name], "euler", cap_feats=cap, cap_mask=cmask, **step_kw)

    ways = {"ode": ode, "constant": engine("constant"), "keep100": engine("keep100"), "keep60": engine("keep60"), "keep30": engine("keep30"),
            "T_Bh": engine("T_Bh")}
    if not args.no_host:
        ways.update(host60=host("keep60"), host30=host("keep30"))
    model.forward_with_cfg(z, torch.zeros(2, device=dev), cap, cmask, 4.0, **step_kw)  # engine, weights, the flags a plain forward reads
    eng = model._engine
    info, last = {}, {}
    for name, fn in ways.items():  # warm-up: every shape and graph key of the timed window, twice (eager use, capture)
        fn()
        last[name] = fn()
        torch.cuda.synchronize()
        info[name] = dict(nfe=eng.last_nfe(), eval_rows=eng.last_eval_rows(), layout_flips=eng.get_option("layout_flips"), last_pair=eng.get_option("last_pair"))
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
    t_b, t_bh = st["keep100"]["median"] / n, st["T_Bh"]["median"] / n
    floors = {}
    for name in ("keep100", "keep60", "keep30"):
        gs = int((tables[name] != 1).sum())
        floors[name] = dict(guided=gs, cond_only=n - gs, floor_ms=round(gs * t_b + (n - gs) * t_bh, 3), measured_ms=st[name]["median"],
                            over_floor=round(st[name]["median"] / (gs * t_b + (n - gs) * t_bh), 5))
    out = {"metric": "guidance_schedule_ms_per_trajectory",
           "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} latent {latent}x{latent} B2 euler {args.points}-point grid scale 4",
           "rounds": args.rounds, "ms_per_trajectory": st, "ms_per_nfe": {"T_B": round(t_b, 4), "T_Bh": round(t_bh, 4)},
           "constant_over_ode": round(st["constant"]["median"] / st["ode"]["median"], 5),
           "ode_spread": round((st["ode"]["max"] - st["ode"]["min"]) / st["ode"]["median"], 5),
           "constant_equals_ode": bool(torch.equal(last["constant"], last["ode"])), "intervals": floors, "calls": info,
           "regimes_share_layout": info["keep100"]["last_pair"] == info["T_Bh"]["last_pair"]}
    if not args.no_host:
        out["engine_equals_host"] = {k: bool(torch.equal(last["keep" + k], last["host" + k])) for k in ("60", "30")}
        out["host_over_engine"] = {k: round(st["host" + k]["median"] / st["keep" + k]["median"], 5) for k in ("60", "30")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
