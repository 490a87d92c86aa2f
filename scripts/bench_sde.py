#!/usr/bin/env python3
"""SDE sampling benchmark: Next-DiT-ImageNet 600M (DiT_Llama_600M_patch2, 256^2 -> latent 32 x 32), 4 labels + 4 null rows through
forward_with_cfg (scale 4) - 8 rows, the engine's largest batch (lt_create: max_batch <= 8; the sampler CLI's default of 8 labels + 8 null
rows does not fit one engine call) - diffusion form "sigma", last step "Mean", Euler-Maruyama and Heun.

    python scripts/bench_sde.py [--steps 50] [--repeats 3] [--out profiles/sde/bench_sde.json]

Measures ms per sampler step (wall time of one Sampler.sample_sde call between two device synchronisations / num_steps) of
  (a) engine     the whole trajectory in ONE lt_sample_sde call: one model evaluation per stage, noise uploaded once
  (b) host loop  the SAME Sampler object with solver.use_engine = False: the reference's loop through the model callable - two evaluations
                 per stage, one host-to-device noise copy and ~20 small torch kernels per step
alternating a, b, a, b, ... `--repeats` times each after one warm-up of both.  Both draw the same noise (same seed), and the run checks that
they return the same states.  Prints one JSON line; --out also writes it to a file.  Random-init weights (timing only)."""
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
    ap.add_argument("--steps", type=int, default=50, help="num_steps of the sampler (the CLI default is 250)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--labels", type=int, default=4, help="labels; the batch is twice that (null rows), at most 8 rows")
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
    res = {"bench": "sde", "model": "DiT_Llama_600M_patch2", "latent": [32, 32], "rows": 2 * n, "cfg_scale": 4.0, "diffusion_form": "sigma",
           "last_step": "Mean", "num_steps": args.steps, "repeats": args.repeats, "methods": {}}
    for method in ("Euler", "Heun"):
        fn = Sampler(create_transport("Linear", "velocity", None, None, None)).sample_sde(sampling_method=method, diffusion_form="sigma",
                                                                                          diffusion_norm=1.0, last_step="Mean", last_step_size=0.04,
                                                                                          num_steps=args.steps)

        def run(engine):
            fn.solver.use_engine = engine
            torch.manual_seed(1)
            return fn(z, model.forward_with_cfg, y=y, cfg_scale=4.0)

        _, a0 = timed(lambda: run(True))  # warm-up: engine, weights upload, graphs, pinned noise buffer
        nfe = model._engine.last_nfe()
        _, b0 = timed(lambda: run(False))
        same = all(torch.equal(p, q) for p, q in zip(a0, b0))
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(timed(lambda: run(True))[0] / args.steps)
            tb.append(timed(lambda: run(False))[0] / args.steps)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        stages = 2 if method == "Heun" else 1
        res["methods"][method] = {
            "engine_ms_per_step": [round(v, 3) for v in ta], "host_loop_ms_per_step": [round(v, 3) for v in tb],
            "engine_median": round(med(ta), 3), "host_loop_median": round(med(tb), 3), "speedup_median": round(med(tb) / med(ta), 3),
            "engine_spread": round(max(ta) - min(ta), 3), "host_loop_spread": round(max(tb) - min(tb), 3),
            "lt_last_nfe": nfe, "host_loop_evaluations": 2 * ((args.steps - 1) * stages + 1), "states_equal": same}
    res.update(graph_replays=model._engine.graph_replays(), version=_lib.load().lt_version().decode(), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
