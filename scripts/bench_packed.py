#!/usr/bin/env python3
"""Aspect-ratio buckets benchmark: NextDiT_2B_GQA_patch2, three images at latents 128x128, 104x152 and 152x104 (1024^2, 832x1216, 1216x832:
one pixel budget in three buckets), CFG 4, the 30-point shifted Euler grid.

    python scripts/bench_packed.py [--points 30] [--repeats 3] [--out profiles/packed_cfg/bench_packed.json]

Measures the wall time (ms, between two device synchronisations) of the three trajectories as
  (a) packed       ONE sample_ode_packed call: 6 rows padded to the longest sequence
  (b) sequential   three sample_ode calls of batch 2, one after the other on the same engine (a new prompt each)
alternating a, b, a, b, ... `--repeats` times each after one warm-up of both, then (a) once more per repeat with the engine's
`attention_variant` option forced to 3 (the ping-pong kernel of attention.hip; packed batches then also keep row-major GEMM operands) and
once more under `pair_layout` 0 (the one-wave kernel on row-major operands).  Beside each (a) leg it prints the attention kernel
lt_op_attention_nk_describe names for the shape and whether the engine ran in the pair-layout regime.  Prints the padding ratio B' N_max / sum N_b and one JSON
line; --out also writes it to a file.  Random-init weights (timing only)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import lumina_t2x_amd  # noqa: E402,F401
from lumina_t2x_amd import _lib, models  # noqa: E402
from lumina_t2x_amd.engine import EngineLimits  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "scripts"))
from bench_views import random_init_, timed  # noqa: E402

SIZES = [(128, 128), (104, 152), (152, 104)]


def time_grid(n, shift=4.0):
    t = torch.linspace(0.0, 1.0, n)
    return t / (t + shift - shift * t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--text", type=int, default=128)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = models.NextDiT_2B_GQA_patch2(qk_norm=True, cap_feat_dim=2048).eval().to(dev, torch.bfloat16)
    random_init_(model)
    half = len(SIZES)
    ntok = [(h // 2) * (w // 2) for h, w in SIZES]
    model.engine_limits = EngineLimits(max_batch=2 * half, max_tokens=max(ntok), max_text=args.text)
    zs = [torch.randn(4, h, w, device=dev).to(torch.bfloat16) for h, w in SIZES]
    cap = torch.randn(2 * half, args.text, 2048, device=dev).to(torch.bfloat16)
    mask = torch.ones(2 * half, args.text, dtype=torch.int32, device=dev)
    mask[half:, 8:] = 0
    pairs = [(torch.stack([z, z]), cap[[b, half + b]].contiguous(), mask[[b, half + b]].contiguous()) for b, z in enumerate(zs)]
    tgrid = time_grid(args.points)
    kw = dict(cfg_scale=4.0, proportional_attn=True, base_seqlen=4096)

    def packed():
        return model.sample_ode_packed(zs + zs, tgrid, cap, mask, method="euler", **kw)

    def sequential():
        outs = []
        for z2, c2, m2 in pairs:
            eng = model.engine(z2, c2.shape[1])
            eng.prepare_prompt(c2, m2)
            outs.append(eng.sample_ode(z2, tgrid, "euler", use_cfg=True, return_trajectory=False, **kw))
        return outs

    _, pa = timed(packed)  # warm-up: engine, weight upload, graphs
    _, pb = timed(sequential)
    eng = model._engine
    L = _lib.load()

    def leg_kernel(name):
        """the attention kernel of the packed self-attention call under the engine's current options, and the operand layout regime of its last evaluation"""
        buf = C.create_string_buffer(64)
        opts = ("attention_variant",)
        saved = {n: eng.get_option(n) for n in opts}
        glob = {}
        for n in opts:  # the describe entry reads the process defaults: mirror the engine's values for the question
            v = C.c_int32(0)
            _lib.check(L.lt_engine_get_option(None, n.encode(), C.byref(v)), n)
            glob[n] = v.value
            _lib.check(L.lt_set_option(n.encode(), saved[n]), n)
        try:
            _lib.check(L.lt_op_attention_nk_describe(0, 0, 2 * half, model.n_heads, model.n_kv_heads, max(ntok), max(ntok), max(ntok), model.dim // model.n_heads,
                                                     1, 1, (args.text + 63) // 64 * 64, buf, 64), "describe")
        finally:
            for n in opts:
                _lib.check(L.lt_set_option(n.encode(), glob[n]), n)
        info = {"attention": buf.value.decode(), "last_pair": eng.get_option("last_pair")}
        print(f"leg {name}: attention kernel {info['attention']}, pair-layout regime {info['last_pair']}")
        return info

    ta, tb, tc, td = [], [], [], []
    for _ in range(args.repeats):
        ta.append(timed(packed)[0])
        tb.append(timed(sequential)[0])
    timed(packed)
    legs = {"packed": leg_kernel("(a) packed")}
    eng.set_option("attention_variant", 3)
    try:
        timed(packed)
        for _ in range(args.repeats):
            tc.append(timed(packed)[0])
        legs["packed_attention_variant_3"] = leg_kernel("(a) packed, attention_variant 3")
    finally:
        eng.set_option("attention_variant", None)
    eng.set_option("pair_layout", 0)
    try:
        timed(packed)
        for _ in range(args.repeats):
            td.append(timed(packed)[0])
        legs["packed_pair_layout_0"] = leg_kernel("(a) packed, pair_layout 0")
    finally:
        eng.set_option("pair_layout", None)
    ratio = half * max(ntok) / sum(ntok)
    print(f"padding ratio B' N_max / sum N_b = {half} x {max(ntok)} / {sum(ntok)} = {ratio:.4f}")
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rel = [float((pa[b].float() - pb[b][0].float()).norm() / pb[b][0].float().norm()) for b in range(half)]
    res = {"bench": "packed_cfg", "model": "NextDiT_2B_GQA_patch2", "latents": SIZES, "tokens": ntok, "padding_ratio": round(ratio, 4), "cfg_scale": 4.0,
           "method": "euler", "grid_points": args.points, "repeats": args.repeats,
           "packed_ms": [round(v, 2) for v in ta], "sequential_ms": [round(v, 2) for v in tb], "packed_attention_variant_3_ms": [round(v, 2) for v in tc],
           "packed_pair_layout_0_ms": [round(v, 2) for v in td], "packed_pair_layout_0_median": round(med(td), 2),
           "packed_pair_layout_0_spread": round(max(td) - min(td), 2), "legs": legs,
           "packed_median": round(med(ta), 2), "sequential_median": round(med(tb), 2), "packed_attention_variant_3_median": round(med(tc), 2),
           "packed_spread": round(max(ta) - min(ta), 2), "sequential_spread": round(max(tb) - min(tb), 2),
           "packed_attention_variant_3_spread": round(max(tc) - min(tc), 2), "packed_over_sequential": round(med(ta) / med(tb), 4),
           "rel_l2_final_packed_vs_sequential": rel,  # (b) scales the softmax by its own length, (a) by the padded one: equal for the longest only
           "graph_replays": eng.graph_replays(), "version": _lib.load().lt_version().decode(), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
