#!/usr/bin/env python3
"""Smoothed-energy guidance at the headline shape (the 2B Next-DiT with RANDOM weights, B = 2, scale 4, |Q| = 3 of L blocks blurred at sigma),
euler, on one box, interleaved, one JSON line per latent size:

    full      lt_sample_ode_cfg_schedule, every entry 4                          - the existing call, same build: the yardstick
    pag       lt_sample_ode_cfg_pag, every entry (w, s) = (4, 2.8), P = the set   - the third evaluation leaves the set's N x N attention out
    seg       lt_sample_ode_cfg_seg, every entry (w, s) = (4, 2.8), Q = the set   - the third evaluation runs the set's blocks in full, on
              queries blurred by query_blur_taps_kernel, with the text launch on top
    host      transport.guidance.sample_cfg_seg stepped from Python on the same model (the definition; ``--host_rounds``, 0: left out)

Every way is timed ``--rounds`` times, the ways alternating inside a round.  Reported per way: ms per trajectory (median, min, max),
``lt_last_nfe`` / ``lt_last_eval_rows``; the measured ratios seg / full and seg / pag beside the ratio DERIVED from rows, 1.5 (a guided stage's
2 B' rows plus B' rows of the third evaluation) - a derivation, not a measurement.  Then the blur kernel alone (lt_op_query_blur on the third
evaluation's query image, [1, H, N, hd]) beside a device-to-device copy of the same bytes, HIP events around ``--kernel_reps`` launches each,
in the same run.  A grid that cannot reflect the radius of ``--sigma`` (256^2 is 16 x 16 tokens: radius <= 15) runs the largest sigma it can,
and says so.  Random weights: nothing here says anything about image quality.

    python scripts/bench_seg.py [--latents 128 32] [--sigma 10] [--points 11] [--rounds 5] [--host_rounds 1] [--small]

Needs a GPU; not part of the test suite.  --small runs a 4-layer model with one block blurred (a functional check of this script)."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import bench  # noqa: E402
import lumina_t2x_amd  # noqa: E402,F401
from lumina_t2x_amd import _lib, models  # noqa: E402
from lumina_t2x_amd.transport import guidance as G  # noqa: E402
from lumina_t2x_amd.transport.mini import ODE  # noqa: E402


def event_ms(fn, reps):
    """ms per call of fn, HIP events around `reps` back-to-back calls (after two warm-up calls)"""
    fn(); fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_vs_copy(H, hd, tokens_side, sigma, reps, gen):
    lib = _lib.load()
    N = tokens_side * tokens_side
    q = torch.randn(1, H, N, hd, device="cuda", generator=gen).to(torch.bfloat16)
    out = torch.empty_like(q)
    mode, r, taps = G.seg_taps(sigma)
    tp = taps.cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def blur():
        rc = lib.lt_op_query_blur(q.data_ptr(), out.data_ptr(), tp.data_ptr() if mode == 0 else None, 1, H, N, hd, tokens_side, tokens_side, r, mode, stream)
        assert rc == 0, lib.lt_last_error()

    t_blur = event_ms(blur, reps)
    t_copy = event_ms(lambda: out.copy_(q), reps)
    nbytes = 2 * q.numel() * 2
    return dict(shape=[1, H, N, hd], radius=r, mode=mode, blur_us=round(t_blur * 1e3, 2), copy_us=round(t_copy * 1e3, 2),
                blur_over_copy=round(t_blur / t_copy, 2), bytes_read_plus_written=nbytes, blur_gb_per_s=round(nbytes / t_blur / 1e6, 1),
                copy_gb_per_s=round(nbytes / t_copy / 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latents", type=int, nargs="+", default=[128, 32])
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--points", type=int, default=11)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host_rounds", type=int, default=1)
    ap.add_argument("--kernel_reps", type=int, default=50)
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
    fours, third = torch.full((n,), 4.0), torch.full((n,), 2.8)
    for latent in args.latents:
        side = latent // model.patch_size
        sigma = args.sigma
        if G.seg_taps(sigma)[1] > side - 1:     # the grid cannot reflect this radius: the widest blur it can
            sigma = (side - 1) / 3.0
        z = torch.randn(1, 4, latent, latent, device=dev, generator=g).to(torch.bfloat16).repeat(2, 1, 1, 1)
        model.forward_with_cfg(z, torch.zeros(2, device=dev), cap, cmask, 4.0, **step_kw)  # engine, weights, the flags a plain forward reads
        eng = model._engine
        sched = lambda **kw: model.sample_ode_cfg_schedule(z, tgrid, fours, cap, cmask, method=method, **kw, **step_kw)
        ways = {"full": lambda: sched(), "pag": lambda: sched(pag=third, pag_layers=layers),
                "seg": lambda: sched(seg=third, seg_layers=layers, seg_sigma=sigma)}
        info, last = {}, {}
        for name, fn in ways.items():  # warm-up: every shape and graph key of the timed window, twice (eager use, capture)
            fn()
            last[name] = fn()
            torch.cuda.synchronize()
            info[name] = dict(nfe=eng.last_nfe(), eval_rows=eng.last_eval_rows(), last_pair=eng.get_option("last_pair"))
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
                states = G.sample_cfg_seg(model, z, tgrid, fours, third, layers, sigma, (), method, cap_feats=cap, cap_mask=cmask, **step_kw)
                torch.cuda.synchronize()
                ms["host"].append((time.perf_counter() - t0) * 1e3)
            ms["host"] = ms["host"][1:]
            host_same = bool(torch.equal(states[-1], last["seg"]))
            model.forward_with_cfg(z, torch.zeros(2, device=dev), cap, cmask, 4.0, **step_kw)

        def stat(vs):
            s = sorted(vs)
            return dict(median=round(s[len(s) // 2], 3), min=round(s[0], 3), max=round(s[-1], 3))

        st = {k: stat(v) for k, v in ms.items()}
        full = last["full"].float()
        kern = kernel_vs_copy(model.n_heads, model.dim // model.n_heads, side, sigma, args.kernel_reps, g)
        out = {"metric": "seg_ms_per_trajectory",
               "shape": f"{'small' if args.small else 'NextDiT_2B_patch2'} random weights, latent {latent}x{latent} B2 {method} {args.points}-point "
                        f"grid ({n} stages) w 4 s 2.8, layers {layers} of {L}",
               "sigma_asked": args.sigma, "sigma_run": round(sigma, 4), "radius": kern["radius"], "token_grid": [side, side],
               "rows_per_evaluation": {"guided": 2 * side ** 2, "third": side ** 2},
               "rounds": args.rounds, "ms_per_trajectory": st, "calls": info,
               "seg_over_full_measured": round(st["seg"]["median"] / st["full"]["median"], 5),
               "pag_over_full_measured": round(st["pag"]["median"] / st["full"]["median"], 5),
               "seg_over_pag_measured": round(st["seg"]["median"] / st["pag"]["median"], 5),
               "seg_over_full_derived_from_rows": 1.5,
               "blur_kernel_vs_device_copy": kern,
               "blur_share_of_seg_trajectory": round(kern["blur_us"] * 1e-3 * len(layers) * n / st["seg"]["median"], 5),
               "host_over_seg": round(st["host"]["median"] / st["seg"]["median"], 5) if "host" in st else None,
               "host_final_state_equals_engine": host_same,
               "rel_l2_from_full_guidance": round(float((last["seg"].float() - full).norm() / full.norm()), 6),
               "full_spread": round((st["full"]["max"] - st["full"]["min"]) / st["full"]["median"], 5)}
        assert math.isfinite(out["rel_l2_from_full_guidance"])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
