"""Launch census of one model evaluation per route of the transformer block.

The routes a block can take (small-fused attention, one q / k / V post-processing launch, the q / k pair kernel, the fused QKV launch with
raw queries and the pair layout, ...) are bit-identical by design, so a comparison of output words cannot tell which one ran.  The
engine's profile can: every launch bracket counts into its kernel class (0 GEMM, 1 attention, 2 other; lt_profile_read), and the flop
tally of the GEMM and attention classes follows the launches' shapes.  This script runs ONE eager evaluation per configuration with the
profile on and records, per class, the bracket count and the flops, plus `last_pair` (lt_engine_get_option) and - where the call is a
sampler call - `layout_flips`.

    python scripts/launch_census.py --out profiles/run_forward_split/launch_census.json      # record
    LUMINA_DIT_LIB=/path/to/other/liblumina_dit.so python scripts/launch_census.py --out ...  # ... the same for another build

tests/test_gpu_launch_census.py asserts the committed table against the library under test.  The shapes are the smallest that reach each
route; the wide engine (two layers at the 2B model's width, 2 x 4096 tokens) is there because the fused QKV launch, raw queries and the
pair layout need one 256-row GEMM tile per CU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import lumina_t2x_amd  # noqa: E402,F401
from lumina_t2x_amd import models  # noqa: E402
from lumina_t2x_amd.engine import EngineLimits  # noqa: E402
from oracle import synth  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
TABLE = os.path.join(REPO, "profiles", "run_forward_split", "launch_census.json")
WIDE = synth.NextDiTConfig(n_layers=2, cap_feat_dim=128)  # d 2304, 32 heads of 72, F 6144: the 2B model's block, twice


def _build(ctor, cfg, seed, streams=False):
    m = ctor(**cfg.ctor_kwargs())
    m.load_state_dict(synth.synth_state_dict(cfg, seed=seed, streams=streams), strict=True)
    return m.eval().to("cuda", torch.bfloat16)


def _measure(eng, call, sampler=False):
    """`call` once unprofiled (engine built, conditioning prepared, weights in the layout the call wants), then once eagerly with the profile on"""
    call()
    torch.cuda.synchronize()
    eng.profile_enable(True)
    try:
        eng.profile_reset()
        call()
        torch.cuda.synchronize()
        reads = [eng.profile_read(k) for k in range(3)]
    finally:
        eng.profile_enable(False)
    row = {"launches": [int(n) for _, n, _ in reads], "flops": [float(f) for _, _, f in reads], "last_pair": eng.get_option("last_pair")}
    if sampler:
        row["layout_flips"] = eng.get_option("layout_flips")
    return row


def _with_options(eng, opts, fn):
    try:
        for n, v in opts.items():
            eng.set_option(n, v)
        return fn()
    finally:
        for n in opts:
            eng.set_option(n, None)


def _text_inputs(cfg, latent_hw, seed=1):
    z, t, cap, mask = synth.synth_inputs(cfg, latent_hw=latent_hw, seed=seed)
    return z.to("cuda", torch.bfloat16), t.cuda(), cap.to("cuda", torch.bfloat16), mask.cuda()


def _label_inputs(cfg, latent_hw, seed=1):
    z, t, y = synth.synth_inputs(cfg, latent_hw=latent_hw, seed=seed)
    return z.to("cuda", torch.bfloat16), t.cuda(), y.cuda()


def census_class_conditional(out):
    """hd 48 at 64 tokens: the small-M QKV GEMM with the one-launch q / k / V post-processing + attention behind it; the MoE families"""
    for name, ctor, cfg in (("imagenet_64tok_small_fused", models.imagenet.DiT_Llama, synth.TINY_IMAGENET),
                            ("moe_time_and_space_64tok", models.moe.DiT_Llama, synth.TINY_MOE),
                            ("moe_time_64tok", models.moe.DiT_Llama_TimeMoE, synth.TINY_MOE_TIME),
                            ("moe_space_64tok", models.moe.DiT_Llama_SpaceMoE, synth.TINY_MOE_SPACE)):
        model = _build(ctor, cfg, 3)
        z, t, y = _label_inputs(cfg, (16, 16))
        call = lambda: model.forward_with_cfg(z, t, y, 4.0)  # noqa: E731
        call()
        out[name] = _measure(model._engine, call)
        if name.startswith("imagenet"):
            out["imagenet_64tok_attn_small_fused_0"] = _with_options(model._engine, {"attn_small_fused": 0}, lambda: _measure(model._engine, call))


def census_text_tiny(out):
    """d 576, hd 72, two layers: below and from 2048 rows, a layer-skip set, the parts of a step-cached evaluation, packed batches"""
    cfg = synth.TINY
    model = _build(models.NextDiT, cfg, 3)
    kw = dict(proportional_attn=True, base_seqlen=16)
    z, t, cap, mask = _text_inputs(cfg, (16, 16))
    call = lambda: model.forward_with_cfg(z, t, cap, mask, 4.0, **kw)  # noqa: E731
    call()
    eng = model._engine
    out["text_128rows_qkv_post"] = _measure(eng, call)
    out["text_128rows_qkv_post_fused_0"] = _with_options(eng, {"qkv_post_fused": 0}, lambda: _measure(eng, call))
    out["text_128rows_plain_forward"] = _measure(eng, lambda: model(z, t, cap, mask))
    out["text_128rows_skip_layer_1"] = _measure(eng, lambda: model(z, t, cap, mask, skip_layers=(1,)))
    # step caching, part by part: the head (probe), the block stack + tail (run), the kept residual + tail (reuse)
    ekw = dict(use_cfg=True, cfg_scale=4.0, **kw)
    out["text_128rows_cache_probe"] = _measure(eng, lambda: eng.forward_cached(z, t, "probe", **ekw))
    out["text_128rows_cache_run"] = _measure(eng, lambda: (eng.forward_cached(z, t, "probe", **ekw), eng.profile_reset(), eng.forward_cached(z, t, "run", **ekw)))
    out["text_128rows_cache_reuse"] = _measure(eng, lambda: (eng.forward_cached(z, t, "probe", **ekw), eng.profile_reset(), eng.forward_cached(z, t, "reuse", **ekw)))
    # packed batches of unequal sizes: the flat form (guided) and the list form (plain forward); 64, 48 and 48 tokens
    gen = torch.Generator().manual_seed(7)
    xs = [torch.randn(cfg.in_channels, h, w, generator=gen).to("cuda", torch.bfloat16) for h, w in ((16, 16), (16, 12), (12, 16))]
    z3, t3, cap3, mask3 = _text_inputs(cfg, (16, 16), seed=2)
    cap6, mask6, t6 = cap3.repeat_interleave(3, 0).contiguous(), mask3.repeat_interleave(3, 0).contiguous(), t3.repeat_interleave(3, 0).contiguous()
    packed = _build(models.NextDiT, cfg, 3)
    pcall = lambda: packed.forward_with_cfg_packed(xs + [x.clone() for x in xs], t6, cap6, mask6, 4.0, **kw)  # noqa: E731
    pcall()
    out["text_packed_64_48_48tok_cfg_flat"] = _measure(packed._engine, pcall)
    th, caph, maskh = t6[:3].contiguous(), cap6[:3].contiguous(), mask6[:3].contiguous()
    lcall = lambda: packed(xs, th, caph, maskh)  # noqa: E731
    lcall()
    out["text_packed_64_48_48tok_list"] = _measure(packed._engine, lcall)
    # 2 x 1024 tokens = 2048 rows: q and k in one persistent launch, V through the transpose kernel
    big = _build(models.NextDiT, cfg, 3)
    zb, tb, capb, maskb = _text_inputs(cfg, (64, 64))
    bcall = lambda: big.forward_with_cfg(zb, tb, capb, maskb, 4.0, proportional_attn=True, base_seqlen=256)  # noqa: E731
    bcall()
    out["text_2048rows_qk_pair"] = _measure(big._engine, bcall)
    out["text_2048rows_qk_post_pair_0"] = _with_options(big._engine, {"qk_post_pair": 0}, lambda: _measure(big._engine, bcall))


def census_regional(out):
    g = np.load(os.path.join(GOLDEN, "compositional_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    model = _build(models.compositional.NextDiT, cfg, int(g["seed_w"]))
    z, t = torch.from_numpy(g["z"]).to("cuda", torch.bfloat16), torch.from_numpy(g["t"]).cuda()
    cap, mask = torch.from_numpy(g["cap"]).to("cuda", torch.bfloat16), torch.from_numpy(g["mask"]).cuda()
    gcap, gmask = torch.from_numpy(g["gcap"]).to("cuda", torch.bfloat16), torch.from_numpy(g["gmask"]).cuda()
    hs, ws = (int(v) for v in g["splits"])
    call = lambda: model.forward_with_cfg(z, t, cap, mask, 4.0, base_seqlen=16, proportional_attn=True, global_cap_feats=gcap,  # noqa: E731
                                          global_cap_mask=gmask, h_split_num=hs, w_split_num=ws)
    call()
    out["text_regional_prompt"] = _measure(model._engine, call)


def census_flag(out):
    """hd 96, 1-D RoPE, one eol token per latent row: 8 x (12 + 1) = 104 tokens"""
    cfg = synth.TINY_FLAG
    model = _build(models.flag_dit.DiT_Llama, cfg, 3)
    z, t, cap, mask = _text_inputs(cfg, (16, 24))
    call = lambda: model.forward_with_cfg(z, t, cap, mask, 4.0, proportional_attn=True, base_seqlen=16)  # noqa: E731
    call()
    out["flag_104tok_eol"] = _measure(model._engine, call)


def census_wide(out):
    """two layers at the 2B width, 2 x 4096 tokens = 8192 rows: the fused QKV launch, raw queries, the pair layout - and each switched off"""
    model = _build(models.NextDiT, WIDE, 3, streams=True)
    model.engine_limits = EngineLimits(max_batch=2, max_tokens=4096, max_text=16)
    z, t, cap, mask = _text_inputs(WIDE, (128, 128))
    kw = dict(proportional_attn=True, base_seqlen=1024)
    call = lambda: model.forward_with_cfg(z, t, cap, mask, 4.0, **kw)  # noqa: E731
    call()
    eng = model._engine
    out["wide_8192rows_fused_qkv_raw_q_pair"] = _measure(eng, call)
    for opt in ("qkv_fused_gemm", "attn_q_fused", "qkv_vt_epilogue", "pair_layout"):
        out[f"wide_8192rows_{opt}_0"] = _with_options(eng, {opt: 0}, lambda: _measure(eng, call))
    # the weights are row-major now (pair_layout 0 came last): one Euler step under the default options converts them once
    _with_options(eng, {"pair_layout": 0}, call)
    tgrid = torch.tensor([0.0, 1.0])
    scall = lambda: eng.sample_ode(z, tgrid, "euler", use_cfg=True, cfg_scale=4.0, **kw)  # noqa: E731
    eng.profile_enable(True)
    try:
        eng.profile_reset()
        scall()
        torch.cuda.synchronize()
        reads = [eng.profile_read(k) for k in range(3)]
    finally:
        eng.profile_enable(False)
    out["wide_8192rows_euler_step_from_row_major"] = {"launches": [int(n) for _, n, _ in reads], "flops": [float(f) for _, _, f in reads],
                                                     "last_pair": eng.get_option("last_pair"), "layout_flips": eng.get_option("layout_flips")}


GROUPS = {"class_conditional": census_class_conditional, "text_tiny": census_text_tiny, "regional": census_regional, "flag": census_flag,
          "wide": census_wide}


def census(group):
    out = {}
    with torch.no_grad():
        GROUPS[group](out)
    return out


def write_table(table, path):
    """JSON, one line per configuration"""
    what = "per kernel class (0 GEMM, 1 attention, 2 other): launch brackets and flops of one eager evaluation (scripts/launch_census.py), by group of configurations"
    groups = []
    for group in sorted(table):
        rows = ",\n".join(f"   {json.dumps(name)}: {json.dumps(table[group][name], sort_keys=True)}" for name in sorted(table[group]))
        groups.append(f"  {json.dumps(group)}: {{\n{rows}\n  }}")
    with open(path, "w") as f:
        f.write("{\n \"what\": " + json.dumps(what) + ",\n \"configs\": {\n" + ",\n".join(groups) + "\n }\n}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=TABLE)
    args = ap.parse_args()
    table = {group: census(group) for group in GROUPS}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    write_table(table, args.out)
    for group in table.values():
        for name, row in sorted(group.items()):
            print(name, row["launches"], "last_pair", row["last_pair"], "layout_flips", row.get("layout_flips"))


if __name__ == "__main__":
    main()
