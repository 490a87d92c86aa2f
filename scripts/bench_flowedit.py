#!/usr/bin/env python3
"""Prompt-driven editing (FlowEdit) on the 2B Next-DiT with RANDOM weights, B' = 1 (4 rows per evaluation), bf16, time shift 4, on one
box, the ways alternating inside a round, one JSON line:

    engine     lt_sample_flowedit: the whole edit in one call
    stepped    the same loop stepped from Python (transport.edit.sample_flowedit) around the engine-backed model's plain forward
    ode4       the yardstick that exists without this feature: lt_sample_ode with use_cfg = 0, euler, batch 4, same grid and shape

Reported: ms per trajectory per way (median, min, max), engine / ode4 and engine / stepped, the spread of ode4 between rounds, ``lt_last_nfe``,
``lt_last_eval_rows`` and the ``layout_flips`` option of each engine call, and whether engine and stepped agree bit for bit.  Random weights:
nothing here says anything about edit quality.

    python scripts/bench_flowedit.py [--latent 128] [--points 30] [--rounds 3] [--small]

Needs a GPU; not part of the test suite.  --small runs a 2-layer model (a functional check of this script)."""
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
from lumina_t2x_amd.transport import edit as E  # noqa: E402
from lumina_t2x_amd.transport.mini import ODE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--points", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
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
    cap = torch.randn(4, bench.TEXT_LEN, 2048, device=dev, generator=g).to(torch.bfloat16)
    cmask = torch.ones(4, bench.TEXT_LEN, dtype=torch.int32, device=dev)
    cmask[2:, 8:] = 0
    tgrid = ODE(args.points, "euler", 4).t
    n = len(tgrid) - 1
    x = torch.randn(1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16)
    noise = torch.randn(n, 1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16)
    step_kw = dict(proportional_attn=True, base_seqlen=(1024 // 16) ** 2)
    scales = E.flowedit_scales(n, 1.5, 5.5)
    z4 = x.repeat(4, 1, 1, 1)

    def engine():
        return model.sample_flowedit(x, tgrid, noise, cap, cmask, src_cfg=1.5, tgt_cfg=5.5, **step_kw)

    def stepped():
        return E.sample_flowedit(model.forward, x, tgrid, noise, scales, cap_feats=cap, cap_mask=cmask)[-1]

    def ode4():
        return ODE(args.points, "euler", 4).sample(z4, model.forward, cap_feats=cap, cap_mask=cmask)[-1]

    ways = {"engine": engine, "stepped": stepped, "ode4": ode4}
    engine()  # engine, weights, the flags the plain forward reads
    eng = model._engine
    info, last = {}, {}
    for name, fn in ways.items():  # warm-up: every shape and graph key of the timed window, twice (eager use, capture)
        fn()
        last[name] = fn()
        torch.cuda.synchronize()
        info[name] = dict(nfe=eng.last_nfe(), eval_rows=eng.last_eval_rows(), layout_flips=eng.get_option("layout_flips"))
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
    out = {"metric": "flowedit_ms_per_trajectory",
           "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} random weights, latent {latent}x{latent} B'=1 (4 rows) euler {args.points}-point "
                    f"grid ({n} intervals) bf16 shift 4",
           "rows_per_evaluation": 4 * (latent // 2) ** 2, "rounds": args.rounds, "ms_per_trajectory": st,
           "ms_per_interval": {k: round(v["median"] / n, 4) for k, v in st.items()},
           "engine_over_ode4": round(st["engine"]["median"] / st["ode4"]["median"], 5),
           "engine_over_stepped": round(st["engine"]["median"] / st["stepped"]["median"], 5),
           "ode4_spread": round((st["ode4"]["max"] - st["ode4"]["min"]) / st["ode4"]["median"], 5),
           "calls": info, "engine_equals_stepped": bool(torch.equal(last["engine"], last["stepped"]))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
