#!/usr/bin/env python3
"""Phase Upscale (visual-anagram) benchmark: NextDiT 2B, 2048^2 (latent 256 x 256 = 16 384 tokens per row), CFG 4, V = 2 views, the anagram
fork's attention rule with proportional attention (base_seqlen 4096) and scale_factor 2.

    python scripts/bench_views_upscale.py [--intervals 2] [--repeats 3] [--latent 256] [--out profiles/views_upscale/bench_views_upscale.json]

Measures ms per time interval of
  (a) one call    ONE lt_sample_views_guided call: per stage one guided gather and one forward_with_cfg of 2 V rows
  (b) per view    the reference's loop (generate.py:465-494) driven from Python over the same engine's forward_with_cfg: per view and stage one
                  evaluation of batch 2, torch ops for the blend, the views and the state arithmetic
alternating a, b, a, b, ... `--repeats` times each after a warm-up of both, wall time between two device synchronisations.  Then the guided
gather kernel alone, as the mean over 200 back-to-back launches between two events.  Prints one JSON line; --out also writes it to a file.
Random-init weights with synthetic statistics (timing only)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "scripts")]

import lumina_t2x_amd  # noqa: E402,F401
from bench_views import random_init_, timed  # noqa: E402
from lumina_t2x_amd import _lib, models, views  # noqa: E402
from lumina_t2x_amd.engine import EngineLimits  # noqa: E402


def per_view(model, vws, caps, mask, z, guidance, grid, kw):
    """generate.py:465-494 with midpoint_solver_extra (:222-262) typed out, one view at a time"""
    V = len(vws)
    noisy, G, Z = z[0].clone(), guidance[0], z[0]
    pairs = [(caps[[v, V + v]].contiguous(), mask[[v, V + v]].contiguous()) for v in range(V)]

    def blend(y, t):
        c = 0.5 * (1 + torch.cos(torch.pi * torch.tensor(t))).cpu()
        return (1 - c) * y + c * (t * G + (1 - t) * Z)

    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = t1 - t0
        half_dt = 0.5 * dt
        inverted = []
        for v, vw in enumerate(vws):
            fn = lambda x, t: model.forward_with_cfg(torch.stack([x] * 2), torch.full((2,), t, device=z.device), pairs[v][0], pairs[v][1], **kw)[0]
            f0 = fn(vw.view(blend(noisy, t0)), t0)
            y_mid = noisy - vw.inverse_view(-f0 * half_dt)
            f1 = fn(vw.view(blend(y_mid, t0 + half_dt)), t0 + half_dt)
            inverted.append(vw.inverse_view(-(f1 * dt)))
        noisy = noisy - torch.stack(inverted).mean(dim=0)
    return noisy[None]


def kernel_us(vws, h, w, n=200):
    lib = _lib.load()
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    V, HW = len(vws), h * w
    perm, vs, isg = (t.cuda() for t in views.stack_tables(vws, h, w))
    y, G, Z = (torch.randn(4, h, w, device="cuda").to(torch.bfloat16) for _ in range(3))
    f = torch.randn(V, 4, h, w, device="cuda").to(torch.bfloat16)
    out = torch.empty_like(f)
    coef = (C.c_float * 4)(0.37, 0.63, 0.16, 0.84)
    res = {}
    for name, f0 in (("guided_gather", None), ("guided_gather_mid", f)):
        call = lambda: lib.lt_op_views_guided_gather(P(y), P(G), P(Z), P(perm), P(vs), P(isg), P(f0), P(out), 0.01, coef, V, 4, HW, _lib.LT_BF16, s)
        for _ in range(20):
            _lib.check(call(), name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) * 1e3 / n, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--views", nargs="+", default=["identity", "rotate_cw"])
    ap.add_argument("--latent", type=int, default=256)
    ap.add_argument("--text_len", type=int, default=128)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = models.NextDiT_2B_patch2(qk_norm=True, cap_feat_dim=2048).eval().to(dev, torch.bfloat16)
    random_init_(model)
    vws = views.get_anagrams_views(args.views)
    V, L = len(vws), args.latent
    z, guidance = (torch.randn(1, 4, L, L, device=dev).to(torch.bfloat16) for _ in range(2))
    caps = torch.randn(2 * V, args.text_len, 2048, device=dev).to(torch.bfloat16)
    mask = torch.ones(2 * V, args.text_len, dtype=torch.int32, device=dev)
    mask[V:, 8:] = 0
    caps[V:] = caps[V]
    t = torch.linspace(0.0, 1.0, args.intervals + 1)
    grid = (t / (t + 4.0 - 4.0 * t)).tolist()
    image = L * 8
    kw = dict(proportional_attn=True, base_seqlen=(1024 // 16) ** 2, scale_factor=max(1.0, image / 1024))
    # one engine for both loops (sized once), the fork's rule on it for the per-view loop's plain forward_with_cfg calls
    model.engine_limits = EngineLimits(2 * V, (L // 2) ** 2, args.text_len)
    eng = model.engine(z.expand(2 * V, -1, -1, -1), args.text_len)
    eng.set_softmax_rule("anagram")
    one = lambda: model.sample_views_guided(z, guidance, grid, vws, caps, mask, cfg_scale=4.0, return_trajectory=False, **kw)
    seq = lambda: per_view(model, vws, caps, mask, z, guidance, grid, dict(kw, cfg_scale=4.0, scale_watershed=0.0))
    _, a0 = timed(one)  # warm-up: weights upload, tables, graphs
    _, b0 = timed(seq)
    timed(one)
    timed(seq)
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(timed(one)[0] / args.intervals)
        tb.append(timed(seq)[0] / args.intervals)
    assert model._engine is eng
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"bench": "views_upscale", "model": "NextDiT_2B_patch2", "latent": [L, L], "tokens_per_row": (L // 2) ** 2, "views": args.views, "cfg_scale": 4.0,
           "intervals": args.intervals, "text_len": args.text_len, "model_kwargs": kw, "one_call_ms_per_interval": [round(v, 2) for v in ta],
           "per_view_ms_per_interval": [round(v, 2) for v in tb], "one_call_median": round(med(ta), 2), "per_view_median": round(med(tb), 2),
           "per_view_spread": round(max(tb) - min(tb), 2), "ratio_per_view_over_one_call": round(med(tb) / med(ta), 3),
           "final_latent_rel_l2_one_call_vs_per_view": float((a0.float() - b0.float()).norm() / b0.float().norm()),
           "nfe_per_interval_one_call": 2, "nfe_per_interval_per_view": 2 * V, "kernel_us": kernel_us(vws, L, L),
           "graph_replays": eng.graph_replays(), "version": _lib.load().lt_version().decode(), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
