#!/usr/bin/env python3
"""Multi-view (visual-anagram) sampling benchmark: NextDiT 2B, 1024^2 (latent 128 x 128 = 4096 tokens), CFG 4, V = 2 views, midpoint.

    python scripts/bench_views.py [--intervals 4] [--repeats 3] [--views identity rotate_cw] [--out profiles/views/bench_views.json]

Measures ms per time interval of
  (a) batched     ONE lt_sample_views call: per stage one forward_with_cfg of 2 V rows (for V = 2 the headline 4 x 4096-row shape)
  (b) sequential  the reference's loop driven from Python on the same engine: per view and stage one forward_with_cfg of batch 2, torch ops
                  for the views and the state arithmetic (uses nothing this feature added to the engine)
alternating a, b, a, b, ... `--repeats` times each after one warm-up of both, wall time between two device synchronisations.  Then the three
view kernels alone (lt_op_views_*), as the mean over 200 back-to-back launches between two events.  Prints one JSON line; --out also writes
it to a file.  Random-init weights with synthetic statistics (timing only)."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import lumina_t2x_amd  # noqa: E402,F401
from lumina_t2x_amd import _lib, models, views  # noqa: E402


def random_init_(model, seed=0):
    """the zero-initialised paths of the architecture (adaLN, gates, final layer) would make every block an identity: fill everything"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("attention.gate"):
                p.normal_(0.0, 0.5, generator=g)
            elif p.dim() == 1 and name.endswith(".weight"):
                p.copy_(1.0 + 0.02 * torch.randn(p.shape, device=p.device, generator=g))
            elif p.dim() == 1:
                p.normal_(0.0, 0.02, generator=g)
            else:
                p.normal_(0.0, min(0.06, p.shape[-1] ** -0.5), generator=g)


def sequential(model, vws, caps, mask, z, grid, cfg_scale):
    V = len(vws)
    noisy = z.repeat(2, 1, 1, 1)
    pairs = [(caps[[v, V + v]].contiguous(), mask[[v, V + v]].contiguous()) for v in range(V)]
    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = t1 - t0
        half_dt = 0.5 * dt
        inverted = []
        for v, vw in enumerate(vws):
            y0 = torch.stack([vw.view(noisy[0])] * 2)
            f0 = model.forward_with_cfg(y0, torch.full((2,), t0, device=z.device), pairs[v][0], pairs[v][1], cfg_scale)
            y_mid = y0 + f0 * half_dt
            noise = -(model.forward_with_cfg(y_mid, torch.full((2,), t0 + half_dt, device=z.device), pairs[v][0], pairs[v][1], cfg_scale) * dt)
            inverted.append(vw.inverse_view(noise[0]))
        noisy = noisy - torch.stack(inverted).mean(dim=0)
    return noisy[:1]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_us(vws, h, w, n=200):
    import ctypes as C
    lib = _lib.load()
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    V, HW = len(vws), h * w
    perm, vs, isg = views.stack_tables(vws, h, w)
    perm, vs, isg = perm.cuda(), vs.cuda(), isg.cuda()
    iperm = torch.empty_like(perm)
    hits = torch.zeros(V * HW + 1, dtype=torch.int32, device="cuda")
    y = torch.randn(4, h, w, device="cuda").to(torch.bfloat16)
    f = torch.randn(V, 4, h, w, device="cuda").to(torch.bfloat16)
    out = torch.empty_like(f)
    red = torch.empty_like(y)
    calls = {
        "invert": lambda: lib.lt_op_views_invert(P(perm), P(iperm), P(hits), V, HW, s),
        "gather": lambda: lib.lt_op_views_gather(P(y), P(perm), P(vs), P(None), P(out), 0.0, V, 4, HW, _lib.LT_BF16, s),
        "gather_mid": lambda: lib.lt_op_views_gather(P(y), P(perm), P(vs), P(f), P(out), 0.01, V, 4, HW, _lib.LT_BF16, s),
        "reduce": lambda: lib.lt_op_views_reduce(P(y), P(f), P(iperm), P(isg), P(red), 0.02, V, 4, HW, _lib.LT_BF16, s),
    }
    res = {}
    for name, call in calls.items():
        for _ in range(20):
            _lib.check(call(), name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) * 1e3 / n, 2)
    res["bytes_moved_per_launch_gather"] = V * 4 * HW * 2 * 2 + V * HW * 4
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--views", nargs="+", default=["identity", "rotate_cw"])
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--text_len", type=int, default=128)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=2048).eval().to(dev, torch.bfloat16)
    random_init_(model)
    vws = views.get_anagrams_views(args.views)
    V = len(vws)
    L = args.latent
    z = torch.randn(1, 4, L, L, device=dev).to(torch.bfloat16)
    caps = torch.randn(2 * V, args.text_len, 2048, device=dev).to(torch.bfloat16)
    mask = torch.ones(2 * V, args.text_len, dtype=torch.int32, device=dev)
    mask[V:, 8:] = 0
    caps[V:] = caps[V]
    t = torch.linspace(0.0, 1.0, args.intervals + 1)
    grid = (t / (t + 4.0 - 4.0 * t)).tolist()
    batched = lambda: model.sample_views(z, grid, vws, caps, mask, "midpoint", cfg_scale=4.0, return_trajectory=False)
    seq = lambda: sequential(model, vws, caps, mask, z, grid, 4.0)
    _, a0 = timed(batched)  # warm-up: engine, weights upload, tables, graphs
    _, b0 = timed(seq)
    timed(batched)
    timed(seq)
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(timed(batched)[0] / args.intervals)
        tb.append(timed(seq)[0] / args.intervals)
    diff = float((a0.float() - b0.float()).norm() / b0.float().norm())
    res = {"bench": "views", "model": "NextDiT_2B_patch2", "latent": [L, L], "views": args.views, "method": "midpoint", "cfg_scale": 4.0,
           "intervals": args.intervals, "text_len": args.text_len, "batched_ms_per_interval": [round(v, 2) for v in ta],
           "sequential_ms_per_interval": [round(v, 2) for v in tb], "batched_median": round(sorted(ta)[len(ta) // 2], 2),
           "sequential_median": round(sorted(tb)[len(tb) // 2], 2), "speedup_median": round(sorted(tb)[len(tb) // 2] / sorted(ta)[len(ta) // 2], 3),
           "final_latent_rel_l2_batched_vs_sequential": diff, "nfe_per_interval_batched": 2, "nfe_per_interval_sequential": 2 * V,
           "view_kernel_us": kernel_us(vws, L, L), "graph_replays": model._engine.graph_replays(),
           "version": _lib.load().lt_version().decode(), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
