#!/usr/bin/env python3
"""Adaptive ODE sampling benchmark: Next-DiT-ImageNet 600M (DiT_Llama_600M_patch2, 256^2 -> latent 32 x 32), 4 labels + 4 null rows through
forward_with_cfg (scale 4), dopri5 at rtol = atol = 2e-2 (the tolerance the project uses for bf16 models: at the reference's defaults any
bf16 model makes the controller chase rounding noise).

    python scripts/bench_ode_adaptive.py [--steps 4] [--repeats 3] [--first-step 0.05] [--out profiles/ode_adaptive/bench_ode_adaptive.json]

Measures ms per ATTEMPTED step (wall time of one Sampler.sample_ode call between two device synchronisations / attempted steps) of
  (a) engine     the whole trajectory in ONE lt_sample_ode_adaptive call: fused stage / error / norm / dense-output kernels, the
                 controller in C++, one 4-byte read per attempted step
  (b) host loop  the SAME Sampler with solver.use_engine = False: adaptive_odeint through the model callable - six Python round trips and
                 ~80 small torch launches per attempted step
alternating a, b, a, b, ... `--repeats` times each after one warm-up of both.  Both start from the same first_step, so both attempt
comparable step sequences (they may still drift apart: the two norms differ in their low bits); the attempt counts of both are reported.
Prints one JSON line; --out also writes it to a file.  Random-init weights (timing only)."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import lumina_t2x_amd  # noqa: E402,F401
from lumina_t2x_amd import _lib, models  # noqa: E402
from lumina_t2x_amd.transport import Sampler, create_transport  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "scripts"))
from bench_views import random_init_, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4, help="grid points of the sampler (the states returned)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--labels", type=int, default=4, help="labels; the batch is twice that (null rows), at most 8 rows")
    ap.add_argument("--first-step", type=float, default=0.05)
    ap.add_argument("--tol", type=float, default=2e-2)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = models.imagenet.DiT_Llama_600M_patch2(qk_norm=True).eval().to(dev, torch.bfloat16)
    random_init_(model)
    n = args.labels
    z = torch.randn(n, 4, 32, 32, device=dev).to(torch.bfloat16)
    z = torch.cat([z, z], 0)
    y = torch.cat([torch.arange(n, device=dev) * 37 % 1000, torch.full((n,), 1000, device=dev)], 0)
    fn = Sampler(create_transport("Linear", "velocity", None, None, None)).sample_ode(sampling_method="dopri5", num_steps=args.steps,
                                                                                       atol=args.tol, rtol=args.tol)
    solver = fn.__self__
    solver.first_step = args.first_step

    def run(engine):
        solver.use_engine = engine
        out = fn(z, model.forward_with_cfg, y=y, cfg_scale=4.0)
        return out, dict(solver.stats)

    _, (a0, sa) = timed(lambda: run(True))  # warm-up: engine, weights upload, graphs, work buffers
    _, (b0, sb) = timed(lambda: run(False))
    ta, tb = [], []
    for _ in range(args.repeats):
        ms, (_, s) = timed(lambda: run(True))
        ta.append(ms / len(s["dt"]))
        ms, (_, s) = timed(lambda: run(False))
        tb.append(ms / len(s["dt"]))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    counts = lambda s: {"attempted": len(s["dt"]), "accepted": s["accepted"], "rejected": s["rejected"], "nfe": s["nfe"]}  # noqa: E731
    res = {"bench": "ode_adaptive", "model": "DiT_Llama_600M_patch2", "latent": [32, 32], "rows": 2 * n, "cfg_scale": 4.0, "method": "dopri5",
           "rtol": args.tol, "atol": args.tol, "first_step": args.first_step, "grid_points": args.steps, "repeats": args.repeats,
           "engine_ms_per_attempted_step": [round(v, 3) for v in ta], "host_loop_ms_per_attempted_step": [round(v, 3) for v in tb],
           "engine_median": round(med(ta), 3), "host_loop_median": round(med(tb), 3), "speedup_median": round(med(tb) / med(ta), 3),
           "engine_spread": round(max(ta) - min(ta), 3), "host_loop_spread": round(max(tb) - min(tb), 3),
           "engine": counts(sa), "host_loop": counts(sb), "same_dt_sequence": sa["dt"] == sb["dt"],
           "rel_l2_last_state": float((a0[-1].float() - b0[-1].float()).norm() / b0[-1].float().norm()),
           "graph_replays": model._engine.graph_replays(), "version": _lib.load().lt_version().decode(),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
