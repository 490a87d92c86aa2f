#!/usr/bin/env python3
"""Multistep ODE sampling at the headline shape (bench.py's cfg2 workload: the 2B Next-DiT, 1024 x 1024, B = 2, time shift 4, scale 4), on one
box, interleaved.  What a user pays is model evaluations (NFE), so the comparison is at equal NFE:

    abm2, abm3   lt_sample_ode_multistep on an N-interval grid                N evaluations
    midpoint     lt_sample_ode on the N/2-interval grid                       N evaluations
    euler        lt_sample_ode on the N-interval grid                         N evaluations
    (ab2, ab3    with --all)

and for each the distance of its final latent from an ``rk4`` run on a 4 x finer grid (16 N evaluations, run once): the relative L2 distance
of the sample (the cond row) in fp32.  The weights are random (timing and the solvers' numerical error on THIS vector field only: no claim
about image quality is made here).  Each way is timed ``--rounds`` times, alternating inside a round; reported: ms per trajectory (median,
min .. max), ``lt_last_nfe`` and the distance.  No threshold is set here.

    python scripts/bench_multistep.py [--intervals 28] [--rounds 3] [--small] [--all] [--out profiles/multistep/bench_multistep.json]

The result carries ``git describe --always --dirty`` of the tree and a hash of the sources that ran (``--tree-hash`` prints both for any
checkout, without a GPU), so a run from a copy without a git directory can still be matched to its tree.  Needs a GPU; not part of the test
suite.  --small runs a 2-layer model at a 64 x 64 latent (a functional check of this script)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bench  # noqa: E402
import lumina_t2x_amd  # noqa: E402,F401
from lumina_t2x_amd import _lib, models  # noqa: E402
from lumina_t2x_amd.transport.mini import ODE  # noqa: E402


def tree_sha256():
    """a hash of the sources that ran - the package, the C ABI headers, bench.py and this script, by path and content - so that a run from a
    copy of the tree without its git directory is still tied to what it ran (``--tree-hash`` prints it for any checkout)"""
    h = hashlib.sha256()
    files = [os.path.join(REPO, "bench.py"), os.path.abspath(__file__)]
    for top in ("lumina-t2x_amd", "include"):
        for root, dirs, names in os.walk(os.path.join(REPO, top)):
            dirs[:] = sorted(d for d in dirs if d not in ("lib", "__pycache__"))
            files += [os.path.join(root, n) for n in names if n.endswith((".py", ".hip", ".h", ".inc")) or n == "Makefile"]
    for path in sorted(files):
        h.update(os.path.relpath(path, REPO).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read() + b"\0")
    return h.hexdigest()[:16]


def commit_stamp():
    """``git describe --always --dirty`` of this tree; without a git directory, the tree hash alone stands for it"""
    try:
        out = subprocess.run(["git", "-C", REPO, "describe", "--always", "--dirty"], capture_output=True, text=True, timeout=10)
        if out.returncode == 0 and out.stdout.strip():
            return out.stdout.strip()
    except (OSError, subprocess.SubprocessError):
        pass
    return "no git directory (see tree_sha256)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=28, help="N: grid intervals of the multistep and euler runs (even; midpoint takes N / 2)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shift", type=float, default=4.0)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--all", action="store_true", help="ab2 and ab3 as well")
    ap.add_argument("--tree-hash", action="store_true", help="print the hash of this tree's sources and exit (no GPU needed)")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "multistep", "bench_multistep.json"))
    args = ap.parse_args()
    if args.tree_hash:
        print(json.dumps({"commit": commit_stamp(), "tree_sha256": tree_sha256()}))
        return
    if args.intervals < 2 or args.intervals % 2:
        ap.error("--intervals must be even and at least 2")
    torch.set_grad_enabled(False)
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
    kw = dict(cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, proportional_attn=True, base_seqlen=(1024 // 16) ** 2, scale_factor=1.0,
              scale_watershed=1.0)
    N = args.intervals
    ways = {"abm2": (N, "abm2"), "abm3": (N, "abm3"), "midpoint": (N // 2, "midpoint"), "euler": (N, "euler")}
    if args.all:
        ways.update(ab2=(N, "ab2"), ab3=(N, "ab3"))
    solvers = {name: ODE(n + 1, method, args.shift) for name, (n, method) in ways.items()}

    def run(name):
        return solvers[name].sample(z, model.forward_with_cfg, **kw)[-1]

    model.forward_with_cfg(z, torch.zeros(2, device=dev), **kw)  # engine, weights, prompt
    eng = model._engine
    ref = ODE(4 * N + 1, "rk4", args.shift).sample(z, model.forward_with_cfg, **kw)[-1][:1].float()
    ref_nfe = eng.last_nfe()
    last, nfe = {}, {}
    for name in ways:  # warm-up: twice (the eager use of a graph key, then its capture)
        run(name)
        last[name] = run(name)
        torch.cuda.synchronize()
        nfe[name] = eng.last_nfe()
    ms = {k: [] for k in ways}
    for _ in range(args.rounds):
        for name in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)

    def stat(vs):
        s = sorted(vs)
        return dict(median=round(s[len(s) // 2], 3), min=round(s[0], 3), max=round(s[-1], 3))

    def dist(x):
        x = x[:1].float()
        return float((x - ref).norm() / ref.norm())

    res = {"bench": "multistep", "commit": commit_stamp(), "tree_sha256": tree_sha256(), "version": _lib.load().lt_version().decode(),
           "device": torch.cuda.get_device_name(0),
           "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} latent {latent}x{latent} B2 bf16 time shift {args.shift} scale 4, random weights",
           "intervals": N, "rounds": args.rounds, "reference": {"method": "rk4", "intervals": 4 * N, "nfe": ref_nfe},
           "ways": {name: {"method": ways[name][1], "intervals": ways[name][0], "nfe": nfe[name], "ms_per_trajectory": stat(ms[name]),
                           "ms_per_nfe": round(stat(ms[name])["median"] / nfe[name], 4), "rel_l2_from_reference": dist(last[name]),
                           "finite": bool(torch.isfinite(last[name].float()).all())} for name in ways}}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
