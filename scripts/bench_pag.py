#!/usr/bin/env python3
"""Perturbed-attention guidance at the headline shape (the 2B Next-DiT with RANDOM weights, B = 2, scale 4, |P| = 3 of L blocks perturbed),
euler, on one box, interleaved, one JSON line per latent size:

    full      lt_sample_ode_cfg_schedule, every entry 4                     - the existing call, same build: the yardstick
    slg       lt_sample_ode_cfg_slg, every entry (w, s) = (4, 2.8), S = the set - the third evaluation launches nothing for the set
    pag       lt_sample_ode_cfg_pag, every entry (w, s) = (4, 2.8), P = the set - the third evaluation runs the set's blocks without the N x N
              attention: V projection [+ Q | K, q post-processing and the text launch], the identity launch, everything behind e->attn
    host      transport.guidance.sample_cfg_pag stepped from Python on the same model (the definition; ``--host_rounds``, 0: left out)

Every way is timed ``--rounds`` times, the ways alternating inside a round.  Reported per way: ms per trajectory (median, min, max),
``lt_last_nfe`` / ``lt_last_eval_rows``, ``layout_flips`` and ``last_pair``; the measured ratios pag / full and pag / slg beside the ratio
DERIVED from rows, 1.5 (a guided stage's 2 B' rows plus B' rows of the third evaluation) - a derivation, not a measurement: PAG has to lie
above SLG (whose set launches nothing) and below 1.5 plus overheads (its set leaves the self-attention out).  Random weights: nothing here
says anything about image quality.

    python scripts/bench_pag.py [--latents 128 32] [--points 11] [--rounds 5] [--host_rounds 2] [--small]

``--latents 128 32`` are 1024^2 and 256^2 images.  Needs a GPU; not part of the test suite.  --small runs a 4-layer model with one block
perturbed (a functional check of this script)."""
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
    ap.add_argument("--latents", type=int, nargs="+", default=[128, 32])
    ap.add_argument("--points", type=int, default=11)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host_rounds", type=int, default=2)
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
    L = model.n_layers
    layers = [1] if args.small else [L // 2 - 1, L // 2, L // 2 + 1]  # three middle blocks
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.randn(2, bench.TEXT_LEN, 2048, device=dev, generator=g).to(torch.bfloat16)
    cmask = torch.ones(2, bench.TEXT_LEN, dtype=torch.int32, device=dev)
    cmask[1, 8:] = 0
    step_kw = dict(proportional_attn=True, base_seqlen=(1024 // 16) ** 2, scale_factor=1.0, scale_watershed=1.0)
    method = "euler"
    tgrid = ODE(args.points, method, 4).t
    n = len(tgrid) - 1
    fours, slg = torch.full((n,), 4.0), torch.full((n,), 2.8)
    for latent in args.latents:
        z = torch.randn(1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16).repeat(2, 1, 1, 1)
        model.forward_with_cfg(z, torch.zeros(2, device=dev), cap, cmask, 4.0, **step_kw)  # engine, weights, the flags a plain forward reads
        eng = model._engine
        ways = {"full": lambda: model.sample_ode_cfg_schedule(z, tgrid, fours, cap, cmask, method=method, **step_kw),
                "slg": lambda: model.sample_ode_cfg_schedule(z, tgrid, fours, cap, cmask, method=method, slg=slg, slg_layers=layers, **step_kw),
                "pag": lambda: model.sample_ode_cfg_schedule(z, tgrid, fours, cap, cmask, method=method, pag=slg, pag_layers=layers, **step_kw)}
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
        host_same = None
        if args.host_rounds > 0:
            ms["host"] = []
            for _ in range(args.host_rounds + 1):  # (the first round warms the per-call keys up and is dropped)
                model.forward_with_cfg(z, torch.zeros(2, device=dev), cap, cmask, 4.0, **step_kw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                states = G.sample_cfg_pag(model, z, tgrid, fours, slg, layers, (), method, cap_feats=cap, cap_mask=cmask, **step_kw)
                torch.cuda.synchronize()
                ms["host"].append((time.perf_counter() - t0) * 1e3)
            ms["host"] = ms["host"][1:]
            host_same = bool(torch.equal(states[-1], last["pag"]))
            model.forward_with_cfg(z, torch.zeros(2, device=dev), cap, cmask, 4.0, **step_kw)

        def stat(vs):
            s = sorted(vs)
            return dict(median=round(s[len(s) // 2], 3), min=round(s[0], 3), max=round(s[-1], 3))

        st = {k: stat(v) for k, v in ms.items()}
        full = last["full"].float()
        out = {"metric": "pag_ms_per_trajectory",
               "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} random weights, latent {latent}x{latent} B2 {method} {args.points}-point "
                        f"grid ({n} stages) w 4 s 2.8, layers {layers} of {L}",
               "rows_per_evaluation": {"guided": 2 * (latent // 2) ** 2, "third": (latent // 2) ** 2},
               "rounds": args.rounds, "ms_per_trajectory": st, "calls": info,
               "pag_over_full_measured": round(st["pag"]["median"] / st["full"]["median"], 5),
               "slg_over_full_measured": round(st["slg"]["median"] / st["full"]["median"], 5),
               "pag_over_slg_measured": round(st["pag"]["median"] / st["slg"]["median"], 5),
               "pag_over_full_derived_from_rows": 1.5,
               "slg_over_full_derived_from_rows": round((2 + (L - len(layers)) / L) / 2, 5),
               "host_over_pag": round(st["host"]["median"] / st["pag"]["median"], 5) if "host" in st else None,
               "host_final_state_equals_engine": host_same,
               "rel_l2_from_full_guidance": round(float((last["pag"].float() - full).norm() / full.norm()), 6),
               "full_spread": round((st["full"]["max"] - st["full"]["min"]) / st["full"]["median"], 5)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
