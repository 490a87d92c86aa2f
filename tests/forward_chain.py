"""One model evaluation of a dense or mixture-of-experts family as a SEQUENCE OF OPERATOR STEPS (plain module, no test in here).

What this is.  `build(case)` turns a reference state-dict, a config and one call's arguments into a list of `Step`s: the conditioning
preparation (cast, mask -> bias, pool + LayerNorm, cap embedder, per layer y-norm / wk_y | wv_y / ky_norm / V transpose; or the label
gather) followed by the evaluation (patchify ... unpatchify with CFG).  Every step names an operator, its operands and its scalar arguments.
The authority for every choice - which norm weight, which modulation chunk, which eps, which scale, which RoPE branch - is the reference's
semantics as oracle/nextdit_oracle.py and oracle/variants_oracle.py restate it (pinned to the unmodified reference by
tests/test_oracle_golden.py); FAMILY below quotes the oracle lines each entry comes from.  It is not written from csrc/engine.hip: the only
thing taken from the engine is WHICH LAUNCH it makes for an operator at these shapes (`paths`), because two launches of one operator may
differ in the summation order of a statistic.

Two backends run the same list:
  Torch64  plain float64 torch on the CPU, written from the operator contracts in include/lumina_dit.h / lumina_dit_debug.h, with no bf16
           rounding inside (the float64 pieces of exact_rows / exact_misc / exact_prologue are reused where they exist);
  Ops      every step is an lt_op_* call on the GPU on buffers of its own: outputs NaN-filled between guard zones (exact_rows.GuardedBuf),
           weights packed here (QKV and wk_y | wv_y concatenated, W1 | W3 through lt_op_pack_w13, every adaLN matrix stacked, the patch
           embedder's K padded to 64).  It never reads engine memory.

Every step's arguments pass through ONE hook, `hook(step_name, args) -> args` (None: the step is left out), so a test changes a single
argument of a single step; `mutations(case)` is the list tests/test_forward_chain_cpu.py and tests/test_gpu_forward_chain.py both run.

Operand references inside `args`:
  ("buf", name)            a buffer of the run                 ("in", name)             an input of the call (x, t, cap, mask, labels)
  ("w", key)               a state-dict tensor                 ("zeros", n)             n zeros
  ("cat", [ref, ...])      rows / elements stacked             ("w13", ref, ref)        the packed W1 | W3 operand of the SwiGLU epilogue
  ("padk", ref, k)         columns zero-padded to k            ("rows", ref, perm)      rows (or elements of a vector) permuted
  ("col", name, off)       d columns of buffer `name` (the modulation matrix) starting at column off, one row per sample
  ("experts13", [(ref, ref), ...])  the experts' packed W1 | W3 operands stacked [E][2F][d]   ("swap2", ref)  the two words of every pair exchanged
  ("forced", layer, branch)         the case's forced routing table of that layer and branch ([rows][2] expert ids), None without one
  ("flipbr", ref)          the two branches of a RoPE table exchanged   ("slots", name[, delta])  the slot count the launch that wrote ystat buffer `name` returned [+ delta]

Mixture-of-experts families.  A routed feed-forward is: router logits -> top-2 + softmax weights (`sel`, `wts`) -> plan (`pos`, `src`,
`te`: kernels.h MoeArgs) -> grouped W1 | W3 GEMM with SwiGLU that gathers its rows of h through `src` -> grouped W2 GEMM -> the closing grn
step, which combines the two experts' rows through `pos` / `wts` in place of reading y.  The time router's logits of ALL layers are one
linear launch on temb (step "t.router"); a layer's plan step reads its E columns and routes.  The space router is a step of its own on h, or
- family `moe`, paths["route_fused"] - the route_* arguments of the grn step that closes the time branch.  The plan buffers of layer l and
branch br are named "sel.l{l}.{br}" ... "te.l{l}.{br}"; both backends keep `sel` readable (Torch64.sel / .logits, Ops.b).
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

import exact_misc as M
import exact_prologue as P64
import exact_rows as R

Step = namedtuple("Step", "name op args")
LOG2E32 = np.float32(1.44269504088896340736)

# The families, from the oracle.  chunk indices: position in `mod.chunk(chunks, dim=1)`; (attention branch, feed-forward branch).
FAMILY = {
    # nextdit_oracle.block: scale_msa, gate_msa, scale_mlp, gate_mlp = mod.chunk(4); x + tanh(gate) * rmsnorm(branch, *_norm2); pre-norm
    # rmsnorm(x, *_norm1) * (1 + scale); forward(): final LayerNorm(1e-6) * (1 + fs), fs the whole final vector; rope_table(): watershed
    "next_t2i": dict(chunks=4, shift=(None, None), scale=(0, 2), gate=(1, 3), tanh=True, pre=("attention_norm1", "ffn_norm1"),
                     post=("attention_norm2", "ffn_norm2"), final=("scale",), text=True, eol=False, rope="2d_watershed", prop=True),
    # variants_oracle.imagenet_block: ch[0] scale, ch[1] gate (tanh), ch[2] scale, ch[3] gate; pf_rmsnorm (no weight) before, rmsnorm(branch,
    # attention_norm / ffn_norm) after; _final_shift_scale: shift, scale = fs.chunk(2); scale sqrt(1 / hd) always; rope_table_2d_general
    "imagenet": dict(chunks=4, shift=(None, None), scale=(0, 2), gate=(1, 3), tanh=True, pre=(None, None), post=("attention_norm", "ffn_norm"),
                     final=("shift", "scale"), text=False, eol=False, rope="2d_general", prop=False),
    # variants_oracle.flag_block: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = mod.chunk(6); x + gate * branch (no tanh, no
    # post-norm); pre-norm rmsnorm(x, attention_norm / ffn_norm); flag_forward: eol token per latent row, rope_table_1d over the flattened row
    # variants_oracle.imagenet_block, family moe_time / moe_space: the imagenet entry with `feed_forward` = ONE MoeLayer - moe_time(sd, p +
    # "feed_forward.", cfg, mod1(pf_rmsnorm(h), ch[2]), time_input, ...) resp. moe_space(... mod1(pf_rmsnorm(h), ch[2]) ...); gated(h, ch[3], f,
    # "ffn_norm.weight").  moe_time: logits = _linear(cond, gate.weight) with cond = time_input = te (imagenet_forward hands `te`, NOT adaln_input,
    # to the blocks), repeated over the sample's tokens; moe_space: logits = _linear(x2, gate.weight) on the FFN input.  _moe_combine: topk(logits,
    # 2), softmax(selected logits) in fp32, results += weight * expert(rows) for e = 0, 1, ...; an expert is feed_forward(): w2(silu(w1 x) * w3 x)
    "moe_time": dict(chunks=4, shift=(None, None), scale=(0, 2), gate=(1, 3), tanh=True, pre=(None, None), post=("attention_norm", "ffn_norm"),
                     final=("shift", "scale"), text=False, eol=False, rope="2d_general", prop=False, moe=(("time", "feed_forward"),)),
    "moe_space": dict(chunks=4, shift=(None, None), scale=(0, 2), gate=(1, 3), tanh=True, pre=(None, None), post=("attention_norm", "ffn_norm"),
                      final=("shift", "scale"), text=False, eol=False, rope="2d_general", prop=False, moe=(("space", "feed_forward"),)),
    # family moe (6 chunks): ft = moe_time(sd, p + "feed_forward_time.", cfg, mod1(pf_rmsnorm(h), ch[2]), time_input, ...); h = gated(h, ch[3], ft,
    # "ffn_norm_time.weight"); fs = moe_space(sd, p + "feed_forward_space.", cfg, mod1(pf_rmsnorm(h), ch[4]), ...) on the UPDATED stream;
    # return gated(h, ch[5], fs, "ffn_norm_space.weight").  scale / gate / post: (attention, first FFN branch, second FFN branch)
    "moe": dict(chunks=6, shift=(None, None, None), scale=(0, 2, 4), gate=(1, 3, 5), tanh=True, pre=(None, None, None),
                post=("attention_norm", "ffn_norm_time", "ffn_norm_space"), final=("shift", "scale"), text=False, eol=False, rope="2d_general",
                prop=False, moe=(("time", "feed_forward_time"), ("space", "feed_forward_space"))),
    "flag_t2i": dict(chunks=6, shift=(0, 3), scale=(1, 4), gate=(2, 5), tanh=False, pre=("attention_norm", "ffn_norm"), post=(None, None),
                     final=("shift", "scale"), text=True, eol=True, rope="1d", prop=True),
}


class Case:
    """one call: the config, the (bf16-valued) state-dict and inputs, and the call's keyword arguments"""

    def __init__(self, cfg, sd, x, t, *, cap=None, mask=None, labels=None, use_cfg=False, cfg_scale=1.0, cfg_channels=3, scale_factor=1.0,
                 scale_watershed=1.0, ntk_factor=1.0, base_seqlen=None, proportional_attn=False, io_dtype=torch.bfloat16, name="", forced=None):
        self.cfg, self.fam, self.name = cfg, FAMILY[cfg.family], name
        r = lambda v: v.detach().cpu().float().to(torch.bfloat16).float()
        self.sd = {k: r(v) for k, v in sd.items()}
        self.inputs = dict(x=r(x), t=t.detach().cpu().float())
        if cap is not None:
            self.inputs.update(cap=r(cap), mask=mask.detach().cpu().to(torch.int32))
        if labels is not None:
            self.inputs["labels"] = labels.detach().cpu().to(torch.int32)
        self.use_cfg, self.cfg_scale, self.cfg_channels = bool(use_cfg), float(cfg_scale), int(cfg_channels)
        self.scale_factor, self.scale_watershed, self.ntk_factor = float(scale_factor), float(scale_watershed), float(ntk_factor)
        self.base_seqlen, self.proportional_attn, self.io_dtype = base_seqlen, bool(proportional_attn), io_dtype
        B, C, H, W = x.shape
        p = cfg.patch_size
        self.B, self.C, self.H, self.W, self.Hp, self.Wp = B, C, H, W, H // p, W // p
        self.Wrow = self.Wp + 1 if self.fam["eol"] else self.Wp
        self.N = self.Hp * self.Wrow
        self.T = cap.shape[1] if cap is not None else 0
        self.forced = None if forced is None else np.ascontiguousarray(forced, dtype=np.int32)     # [L][2: time, space][B * N][2], -1: branch not run


def softmax_scale(case):
    """the self-attention scale, in double, cast once (nextdit_oracle.forward :198-201, flag_forward: N counts the eol tokens; imagenet_block:
    sqrt(1 / head_dim) whatever the call says)"""
    hd = case.cfg.head_dim
    if case.fam["prop"] and case.proportional_attn:
        return float(np.float32(math.sqrt(math.log(case.N, case.base_seqlen) / hd)))
    return float(np.float32(math.sqrt(1.0 / hd)))


def fold(scale):
    """a softmax scale folded into K's one rounding: scores in log2 units, scale x log2(e) as one fp32 product (lt_op_qk_norm_rope out_scale)"""
    return float(np.float32(scale) * LOG2E32)


def build(case, paths=None):
    """-> [Step].  paths: {"small_fused": bool} - which launch pair runs a class-conditional layer's attention (lt_op_qkv_attention_small,
    the default at head_dim 48 / <= 512 tokens, or projection + lt_op_qkv_post + lt_op_attention); {"route_fused": bool} - family moe: the
    space router runs inside the grn step that closes the time branch (the engine's option moe_route_fused, default on) or as a step of its own;
    {"time_plan_hoist": bool} - the engine's option moe_time_plan_hoist: the engine then writes every layer's time plan in one launch; the chain
    plans layer by layer either way (the key is recorded for the tests, the steps do not change).
    The large-row regime of the dense families (from one 256-row tile per CU on; csrc/engine.hip plan_block decides, the tests assert it):
    {"qkv": "plain" | "fused" | "qk_vt"} - one plain projection, lt_op_gemm_qkv (Q | K plain, V as the V^T image only), or Q | K plain plus
    lt_op_gemm_vt; {"raw_q": bool} (with "fused", head_dim 72) - lt_op_qkv_qstat (projection with the Q partial sums + the K pass) and the
    attention that builds its queries itself (lt_op_attention_qraw_ex); {"post": "one" | "pair"} - lt_op_qkv_post, or lt_op_qk_norm_rope_pair
    [+ lt_op_v_transpose behind a plain projection]; {"ystat": 0 | 1} - O and W2 through lt_op_gemm_ystat and every closing step through
    lt_op_gated_residual_norm_ex with the partial sums that launch left.  The float64 meaning of every one of these is that of the default list."""
    paths = {"small_fused": True, "route_fused": True, "time_plan_hoist": True, "qkv": "plain", "raw_q": False, "post": "one", "ystat": 0,
             **(paths or {})}
    assert paths["qkv"] in ("plain", "fused", "qk_vt") and paths["post"] in ("one", "pair") and (not paths["raw_q"] or paths["qkv"] == "fused")
    assert paths["post"] == "pair" or paths["raw_q"] or paths["qkv"] == "plain", "lt_op_qkv_post transposes V itself: a plain projection only"
    large = paths["qkv"] != "plain" or paths["post"] != "one"
    cfg, fam = case.cfg, case.fam
    d, L, H, Hkv, hd, F = cfg.dim, cfg.n_layers, cfg.n_heads, cfg.kv_heads, cfg.head_dim, cfg.ffn_hidden
    A, cap, dkv, ch = min(d, 1024), cfg.cap_feat_dim, cfg.kv_heads * cfg.head_dim, fam["chunks"]
    B, N, T, Tpad, Npad, M_ = case.B, case.N, case.T, -(-case.T // 64) * 64, -(-case.N // 64) * 64, case.B * case.N
    eps = cfg.norm_eps
    cd, fd = ch * d, len(fam["final"]) * d
    ld_mod = L * cd + fd
    w = lambda key: ("w", key)
    buf = lambda name: ("buf", name)
    lw = lambda l, key: None if key is None else ("w", f"layers.{l}.{key}.weight")
    col = lambda l, idx: None if idx is None else ("col", "mod", l * cd + idx * d)
    steps = []
    add = lambda name, op, **args: steps.append(Step(name, op, args))

    # ---- the conditioning, once per prompt / label set --------------------------------------------------------------------------------------
    if fam["text"]:
        add("prep.cast", "cast", src=("in", "cap"), dst="capb", n=B * T * cap)
        add("prep.bias", "mask_to_bias", mask=("in", "mask"), dst="tbias", B=B, T=T, Tpad=Tpad)
        add("prep.pool", "cap_pool_ln", cap=buf("capb"), mask=("in", "mask"), w=w("cap_embedder.0.weight"), b=w("cap_embedder.0.bias"),
            dst="cap_ln", B=B, T=T, C=cap)
        add("prep.cap_embed", "linear", a=buf("cap_ln"), w=w("cap_embedder.1.weight"), b=w("cap_embedder.1.bias"), dst="cap_emb", M=B, N=A, K=cap,
            act=0)
        for l in range(L):
            p = f"layers.{l}.attention."
            add(f"prep.l{l}.ynorm", "rmsnorm_mod", x=buf("capb"), w=lw(l, "attention_y_norm"), scale=None, shift=None, dst="capn", B=B, N=T, d=cap,
                eps=eps, ld_mod=0)
            add(f"prep.l{l}.kvy", "gemm", a=buf("capn"), w=("cat", [w(p + "wk_y.weight"), w(p + "wv_y.weight")]), bias=None, dst=f"kvy{l}", M=B * T,
                N=2 * dkv, K=cap, epi=0, splitk=False)
            add(f"prep.l{l}.ky", "qk_norm", src=buf(f"kvy{l}"), ld=2 * dkv, col0=0, ln_w=w(p + "ky_norm.weight") if cfg.qk_norm else None,
                ln_b=w(p + "ky_norm.bias") if cfg.qk_norm else None, ln_eps=1e-5, dst=f"ky{l}", B=B, N=T, heads=Hkv, hd=hd,
                out_scale=fold(np.float32(1.0 / math.sqrt(hd))))      # F.scaled_dot_product_attention's default scale (oracle attention())
            add(f"prep.l{l}.vty", "v_transpose", src=buf(f"kvy{l}"), ld=2 * dkv, col0=dkv, dst=f"vty{l}", B=B, N=T, Npad=Tpad, kvh=Hkv, hd=hd)
    else:
        add("prep.labels", "label_gather", table=w("y_embedder.embedding_table.weight"), labels=("in", "labels"), dst="cap_emb", B=B,
            rows=cfg.num_classes + 1, d=A)

    # ---- the evaluation -----------------------------------------------------------------------------------------------------------------------
    pp = cfg.patch_size * cfg.patch_size
    add("patchify", "patchify", x=("in", "x"), dst="patches", B=B, C=case.C, H=case.H, W=case.W, patch=cfg.patch_size, kpad=64,
        dup=int(case.use_cfg), wp_stride=case.Wrow if fam["eol"] else 0)
    add("x_embed", "gemm", a=buf("patches"), w=("padk", w("x_embedder.weight"), 64), bias=w("x_embedder.bias"), dst="x", M=M_, N=d, K=64, epi=0,
        splitk=False)
    if fam["eol"]:
        add("eol", "eol_fill", x="x", eol=w("eol_token"), rows_total=B * case.Hp, Wp=case.Wp, d=d)
    add("t.features", "timestep_features", t=("in", "t"), dst="tfeat", B=B, dim=256)
    add("t.mlp0", "linear", a=buf("tfeat"), w=w("t_embedder.mlp.0.weight"), b=w("t_embedder.mlp.0.bias"), dst="t1", M=B, N=A, K=256, act=0)
    add("t.mlp2", "linear", a=buf("t1"), w=w("t_embedder.mlp.2.weight"), b=w("t_embedder.mlp.2.bias"), dst="temb", M=B, N=A, K=A, act=1)
    moe = fam.get("moe", ())
    E = cfg.num_experts if moe else 0
    tiles = (2 * M_ + E * 255 + 255) // 256      # the sorted buffers' tile bound, from the call's rows (kernels.h MoeArgs::max_tiles; moe.hip check())
    forced = lambda l, br: None if case.forced is None else ("forced", l, 0 if br == "time" else 1)
    time_key = next((key for br, key in moe if br == "time"), None)
    add("adaln.add", "add", a=buf("temb"), b=buf("cap_emb"), dst="adaln_in", n=B * A)
    if time_key:     # moe_time(): logits = _linear(cond, gate.weight), cond = te for every layer: ONE launch over the layers' gates stacked
                     # (placed behind adaln.add only so that a mutation can hand it adaln_in; it depends on temb alone)
        add("t.router", "linear", a=buf("temb"), w=("cat", [w(f"layers.{l}.{time_key}.gate.weight") for l in range(L)]), b=None, dst="tlogits", M=B,
            N=L * E, K=A, act=0)
    ada_w = [w(f"layers.{l}.adaLN_modulation.1.weight") for l in range(L)] + [w("final_layer.adaLN_modulation.1.weight")]
    ada_b = [w(f"layers.{l}.adaLN_modulation.1.bias") for l in range(L)] + [w("final_layer.adaLN_modulation.1.bias")]
    add("adaln.linear", "linear", a=buf("adaln_in"), w=("cat", ada_w), b=("cat", ada_b), dst="mod", M=B, N=ld_mod, K=A, act=1)
    tanh_mask = sum(1 << g for g in fam["gate"]) if fam["tanh"] else 0
    add("adaln.prep", "prep_mod", mod="mod", B=B, ld_mod=ld_mod, L=L, chunks=ch, d=d, tanh_mask=tanh_mask, scale_mask=sum(1 << s for s in fam["scale"]),
        final_scale_chunk=fam["final"].index("scale"))
    if fam["rope"] == "2d_watershed":   # nextdit_oracle.rope_table: t < watershed -> positions / scale_factor, else theta * scale_factor
        sf = case.scale_factor
        add("rope", "rope_table", dst="rope", len=384, hd=hd, step=4, theta0=10000.0, lin0=sf, theta1=10000.0 * sf, lin1=1.0, lin_on_pos=0,
            **({"dst_t": "rope_t"} if paths["raw_q"] else {}))
        rope = dict(rope_mode=1, t=("in", "t"), watershed=case.scale_watershed, grid_w=case.Wp, cs_len=384)
    else:                               # rope_table_2d_general / rope_table_1d: theta * ntk_factor, positions / rope_scaling_factor, one table
        th, step = 10000.0 * case.ntk_factor, 2 if fam["rope"] == "1d" else 4
        ln = Npad if fam["rope"] == "1d" else 384
        add("rope", "rope_table", dst="rope", len=ln, hd=hd, step=step, theta0=th, lin0=case.scale_factor, theta1=th, lin1=case.scale_factor,
            lin_on_pos=1, **({"dst_t": "rope_t"} if paths["raw_q"] else {}))
        rope = dict(rope_mode=2 if fam["rope"] == "1d" else 1, t=None, watershed=0.0, grid_w=case.Wp, cs_len=ln)
    add("l0.prenorm", "rmsnorm_mod", x=buf("x"), w=lw(0, fam["pre"][0]), scale=col(0, fam["scale"][0]), shift=col(0, fam["shift"][0]), dst="h", B=B,
        N=N, d=d, eps=eps, ld_mod=ld_mod, scale_pre=1)
    sm = softmax_scale(case)
    for l in range(L):
        p = f"layers.{l}.attention."
        wqkv = ("cat", [w(p + "wq.weight"), w(p + "wk.weight"), w(p + "wv.weight")])
        ln = {k: (w(p + k.replace("_w", ".weight").replace("_b", ".bias")) if cfg.qk_norm else None)
              for k in ("q_norm_w", "q_norm_b", "k_norm_w", "k_norm_b")}
        if not fam["text"] and paths["small_fused"] and not large:
            add(f"l{l}.qkv_attn", "qkv_attention_small", a=buf("h"), w=wqkv, qkv="qkv", M=M_, K=d, H=H, Hkv=Hkv, tokens=N, hd=hd, q_ln_w=ln["q_norm_w"],
                q_ln_b=ln["q_norm_b"], k_ln_w=ln["k_norm_w"], k_ln_b=ln["k_norm_b"], table=buf("rope"), table_len=rope["cs_len"], grid_w=rope["grid_w"],
                k_scale=fold(sm), dst="attn")
        else:
            ld = d + dkv if paths["qkv"] == "qk_vt" else d + 2 * dkv       # the row stride of the buffer that holds Q | K [| V]
            if paths["raw_q"]:     # the projection whose epilogue leaves the Q columns' partial sums, and the K pass that reduces them
                add(f"l{l}.qkv", "qkv_qstat", a=buf("h"), w=wqkv, qkv="qkv", vt="vt", M=M_, N=d + 2 * dkv, K=d, split=d + dkv, tokens=N, hd=hd, q_cols=d,
                    k_ln_w=ln["k_norm_w"], k_ln_b=ln["k_norm_b"], table=buf("rope"), t=rope["t"], watershed=rope["watershed"], grid_w=rope["grid_w"],
                    k_scale=fold(sm), k="k", qmr="qmr")
            elif paths["qkv"] == "fused":
                add(f"l{l}.qkv", "gemm_qkv", a=buf("h"), w=wqkv, qkv="qkv", vt="vt", M=M_, N=d + 2 * dkv, K=d, split=d + dkv, tokens=N, hd=hd)
            elif paths["qkv"] == "qk_vt":
                add(f"l{l}.qkv", "gemm", a=buf("h"), w=("cat", [w(p + "wq.weight"), w(p + "wk.weight")]), bias=None, dst="qkv", M=M_, N=d + dkv, K=d, epi=0,
                    splitk=True)
                add(f"l{l}.v_vt", "gemm_vt", a=buf("h"), w=w(p + "wv.weight"), dst="vt", M=M_, N=dkv, K=d, tokens=N, hd=hd)
            else:
                add(f"l{l}.qkv", "gemm", a=buf("h"), w=wqkv, bias=None, dst="qkv", M=M_, N=d + 2 * dkv, K=d, epi=0, splitk=True)
            if paths["raw_q"]:
                pass
            elif paths["post"] == "pair":
                add(f"l{l}.qk_post", "qk_post_pair", qkv=buf("qkv"), ld=ld, q_col0=0, k_col0=d, q_ln_w=ln["q_norm_w"], q_ln_b=ln["q_norm_b"],
                    k_ln_w=ln["k_norm_w"], k_ln_b=ln["k_norm_b"], ln_eps=1e-5, q="q", k="k", B=B, N=N, H=H, Hkv=Hkv, hd=hd, table=buf("rope"), q_scale=1.0,
                    k_scale=fold(sm), **rope)
                if paths["qkv"] == "plain":
                    add(f"l{l}.v_t", "v_transpose", src=buf("qkv"), ld=ld, col0=d + dkv, dst="vt", B=B, N=N, Npad=Npad, kvh=Hkv, hd=hd)
            else:
                add(f"l{l}.qkv_post", "qkv_post", qkv=buf("qkv"), ld=d + 2 * dkv, q_col0=0, k_col0=d, v_col0=d + dkv, q_ln_w=ln["q_norm_w"],
                    q_ln_b=ln["q_norm_b"], k_ln_w=ln["k_norm_w"], k_ln_b=ln["k_norm_b"], ln_eps=1e-5, q="q", k="k", vt="vt", B=B, N=N, Npad=Npad, H=H,
                    Hkv=Hkv, hd=hd, table=buf("rope"), q_scale=1.0, k_scale=fold(sm), **rope)
            text = dict(tk=buf(f"ky{l}"), tvt=buf(f"vty{l}"), tbias=buf("tbias"), tgate=w(p + "gate"), T=T, Tpad=Tpad) if fam["text"] else {}
            if paths["raw_q"]:     # q_norm + RoPE in the attention's prologue, from the projection's rows; the KERNEL selects the table branch
                none = dict(tk=None, tvt=None, tbias=None, tgate=None, T=0, Tpad=0)
                add(f"l{l}.attn", "attention_qraw", qkv=buf("qkv"), ld=ld, q_col0=0, qmr=buf("qmr"), q_ln_w=ln["q_norm_w"], q_ln_b=ln["q_norm_b"],
                    table=buf("rope"), table_t=buf("rope_t"), table_len=rope["cs_len"], grid_w=rope["grid_w"], t=rope["t"], watershed=rope["watershed"],
                    k=buf("k"), vt=buf("vt"), dst="attn", B=B, H=H, Hkv=Hkv, N=N, Npad=Npad, hd=hd, **(text or none))
            elif fam["text"]:
                add(f"l{l}.attn", "attention_fused", q=buf("q"), k=buf("k"), vt=buf("vt"), dst="attn", B=B, H=H, Hkv=Hkv, N=N, Npad=Npad, hd=hd, **text)
            else:
                add(f"l{l}.attn", "attention", q=buf("q"), k=buf("k"), vt=buf("vt"), dst="attn", B=B, H=H, Hkv=Hkv, N=N, Npad=Npad, hd=hd)
        ys = lambda br: dict(ystat=buf(f"ystat.l{l}.{br}"), ystat_slots=("slots", f"ystat.l{l}.{br}")) if paths["ystat"] else {}
        if paths["ystat"]:
            add(f"l{l}.wo", "gemm_ystat", a=buf("attn"), w=w(p + "wo.weight"), dst="o", ystat=f"ystat.l{l}.o", M=M_, N=d, K=d)
        else:
            add(f"l{l}.wo", "gemm", a=buf("attn"), w=w(p + "wo.weight"), bias=None, dst="o", M=M_, N=d, K=d, epi=0, splitk=True)
        add(f"l{l}.grn_attn", "grn", **ys("o"), x="x", y=buf("o"), post_w=lw(l, fam["post"][0]), gate=col(l, fam["gate"][0]), post_mode=int(fam["post"][0] is not None),
            next_w=lw(l, fam["pre"][1]), next_scale=col(l, fam["scale"][1]), next_shift=col(l, fam["shift"][1]), next_mode=1, ld_mod=ld_mod, h="h", B=B, N=N,
            d=d, eps=eps, eps_next=1e-6)
        for i, (br, key) in enumerate(moe):
            f, nm = f"layers.{l}.{key}.", f"l{l}.{br}"
            plan = {k: f"{k}.{nm}" for k in ("sel", "wts", "pos", "src", "te")}
            if br == "time":
                add(f"{nm}.plan", "moe_plan", logits=buf("tlogits"), sample_ld=L * E, col0=l * E, sel_in=None, forced=forced(l, br), rows=M_, rows_per_sample=N,
                    E=E, max_tiles=tiles, **plan)
            else:
                if not (i == 1 and paths["route_fused"]):      # (fused: the grn step that closed the time branch has routed h already)
                    add(f"{nm}.route", "moe_route", x=buf("h"), gate_w=w(f + "gate.weight"), forced=forced(l, br), rows=M_, rows_per_sample=N, d=d, E=E,
                        max_tiles=tiles, sel=plan["sel"], wts=plan["wts"])
                add(f"{nm}.plan", "moe_plan", logits=None, sample_ld=0, col0=0, sel_in=buf(plan["sel"]), forced=None, rows=M_, rows_per_sample=N, E=E,
                    max_tiles=tiles, **plan)
            add(f"{nm}.w13", "gemm_grouped_gather", a=buf("h"), a_rows=M_, src=buf(plan["src"]), te=buf(plan["te"]),
                w=("experts13", [(w(f + f"experts.{e}.w1.weight"), w(f + f"experts.{e}.w3.weight")) for e in range(E)]), E=E, dst="moe_us", M=tiles * 256,
                N=2 * F, K=d)
            add(f"{nm}.w2", "gemm_grouped", a=buf("moe_us"), te=buf(plan["te"]), w=("cat", [w(f + f"experts.{e}.w2.weight") for e in range(E)]), E=E,
                dst="moe_ys", M=tiles * 256, N=d, K=F)
            if i + 1 < len(moe):     # family moe: the time branch closes, the space branch's pre-norm (no weight) and modulation follow
                nb, nkey = moe[i + 1]
                route = {}
                if paths["route_fused"]:
                    route = dict(route_w=w(f"layers.{l}.{nkey}.gate.weight"), route_E=E, route_sel=f"sel.l{l}.{nb}", route_wts=f"wts.l{l}.{nb}",
                                 route_forced=forced(l, nb))
                add(f"l{l}.grn_{br}", "grn", x="x", y=None, moe_ys=buf("moe_ys"), moe_pos=buf(plan["pos"]), moe_wts=buf(plan["wts"]),
                    post_w=lw(l, fam["post"][1 + i]), gate=col(l, fam["gate"][1 + i]), post_mode=1, next_w=None, next_scale=col(l, fam["scale"][2 + i]),
                    next_shift=None, next_mode=1, ld_mod=ld_mod, h="h", B=B, N=N, d=d, eps=eps, eps_next=1e-6, **route)
        if moe:
            last = dict(y=None, moe_ys=buf("moe_ys"), moe_pos=buf(plan["pos"]), moe_wts=buf(plan["wts"]))
        else:
            last = dict(y=buf("o"))
        f = f"layers.{l}.feed_forward."
        if not moe:
            add(f"l{l}.w13", "gemm", a=buf("h"), w=("w13", w(f + "w1.weight"), w(f + "w3.weight")), bias=None, dst="u", M=M_, N=2 * F, K=d, epi=1, splitk=False)
            if paths["ystat"]:
                add(f"l{l}.w2", "gemm_ystat", a=buf("u"), w=w(f + "w2.weight"), dst="o", ystat=f"ystat.l{l}.f", M=M_, N=d, K=F)
            else:
                add(f"l{l}.w2", "gemm", a=buf("u"), w=w(f + "w2.weight"), bias=None, dst="o", M=M_, N=d, K=F, epi=0, splitk=True)
        if l + 1 < L:
            nxt = dict(next_w=lw(l + 1, fam["pre"][0]), next_scale=col(l + 1, fam["scale"][0]), next_shift=col(l + 1, fam["shift"][0]), next_mode=1)
        else:    # final layer: affine-free LayerNorm, eps 1e-6, * (1 + scale) [+ shift] (forward() :208-211, _final_shift_scale)
            fin = {nm: ("col", "mod", L * cd + i * d) for i, nm in enumerate(fam["final"])}
            nxt = dict(next_w=None, next_scale=fin["scale"], next_shift=fin.get("shift"), next_mode=2)
        add(f"l{l}.grn_ffn", "grn", x="x", post_w=lw(l, fam["post"][-1]), gate=col(l, fam["gate"][-1]), post_mode=int(fam["post"][-1] is not None),
            ld_mod=ld_mod, h="h", B=B, N=N, d=d, eps=eps, eps_next=1e-6, **last, **nxt, **({} if moe else ys("f")))
    nfinal = pp * cfg.out_channels
    add("final.linear", "gemm", a=buf("h"), w=w("final_layer.linear.weight"), bias=w("final_layer.linear.bias"), dst="frows", M=M_, N=nfinal, K=d, epi=0,
        splitk=False)
    add("unpatchify", "unpatchify", rows=buf("frows"), ld=nfinal, dst="out", B=B, C=case.C, out_ch=cfg.out_channels, H=case.H, W=case.W, patch=cfg.patch_size,
        use_cfg=int(case.use_cfg), cfg_scale=case.cfg_scale, cfg_channels=case.cfg_channels, wp_stride=case.Wrow if fam["eol"] else 0, sample_perm=None)
    return steps


def run(backend, steps, hook=None):
    for s in steps:
        args = dict(s.args) if hook is None else hook(s.name, dict(s.args))
        if args is not None:
            backend.step = s.name
            getattr(backend, "op_" + s.op)(**args)
    return backend.result()


# ---- mutations ----------------------------------------------------------------------------------------------------------------------------------
def set_arg(step, **new):
    """hook: the named arguments of ONE step replaced"""
    def hook(name, args):
        if name == step:
            assert all(k in args for k in new), (step, list(new), list(args))
            args.update(new)
        return args
    return hook


def set_everywhere(op_arg, old, new):
    """hook: a value every step shares (a config scalar such as norm_eps): argument `op_arg` where it equals `old`"""
    def hook(name, args):
        if op_arg in args and args[op_arg] == old:
            args[op_arg] = new
        return args
    return hook


def both(*hooks):
    def hook(name, args):
        for h in hooks:
            args = h(name, args)
            if args is None:
                return None
        return args
    return hook


def drop(step):
    return lambda name, args: None if name == step else args


def mutations(case, steps):
    """[(name, hook)]: the wiring mistakes of the issue, each one argument of one step (a swap: the two arguments it exchanges) where the fixture
    has it.  Written against the step list: every entry looks the arguments it changes up in `steps`, so a renamed step fails loudly."""
    cfg, fam = case.cfg, case.fam
    d, L, hd, H = cfg.dim, cfg.n_layers, cfg.head_dim, cfg.n_heads
    by = {s.name: s.args for s in steps}
    cd = fam["chunks"] * d
    out, eps_only = [], []     # eps_only: the LayerNorm eps entries, which only a case with small rows can see (eps_case)
    W = lambda l, key: ("w", f"layers.{l}.{key}.weight")
    zeros = lambda n: ("zeros", n)
    mha = cfg.kv_heads == cfg.n_heads
    fused = "l0.qkv_attn" in by
    for l in range(L):
        # where layer l's first pre-norm runs: the first norm step for layer 0, the closing step of the block before otherwise
        pre_step, pre_arg = ("l0.prenorm", "w") if l == 0 else (f"l{l - 1}.grn_ffn", "next_w")
        if fam["pre"][0]:    # the two pre-norm weights exchanged (attention_norm1 <-> ffn_norm1; Flag-DiT: attention_norm <-> ffn_norm)
            out.append((f"l{l}.pre_norms_swapped", both(set_arg(pre_step, **{pre_arg: W(l, fam["pre"][1])}),
                                                       set_arg(f"l{l}.grn_attn", next_w=W(l, fam["pre"][0])))))
        if fam["post"][0]:   # the two post-norm weights exchanged
            out.append((f"l{l}.post_norms_swapped", both(set_arg(f"l{l}.grn_attn", post_w=W(l, fam["post"][1])),
                                                        set_arg(f"l{l}.grn_ffn", post_w=W(l, fam["post"][0])))))
        qstep = f"l{l}.qkv_attn" if fused else f"l{l}.qkv_post"
        a = by[qstep]
        if mha:
            out.append((f"l{l}.q_k_norm_weight_swapped", set_arg(qstep, q_ln_w=a["k_ln_w"], k_ln_w=a["q_ln_w"])))
        out.append((f"l{l}.q_norm_bias_dropped", set_arg(qstep, q_ln_b=zeros(d))))
        if l > 0:
            if fam["pre"][0]:
                out.append((f"l{l}.reads_layer0_pre_norm", set_arg(pre_step, **{pre_arg: W(0, fam["pre"][0])})))
            else:
                out.append((f"l{l}.reads_layer0_post_norm", set_arg(f"l{l}.grn_attn", post_w=W(0, fam["post"][0]))))
            # every modulation operand of layer l, one at a time, read at layer 0's column: the pre-norm's scale / shift (they sit in the
            # closing step of the block before), both gates, the feed-forward pre-norm's scale / shift
            for step, names in ((pre_step, ("next_scale", "next_shift")), (f"l{l}.grn_attn", ("gate", "next_scale", "next_shift")),
                                (f"l{l}.grn_ffn", ("gate",))):
                for arg in names:
                    c = by[step][arg]
                    if c is not None:
                        out.append((f"l{l}.chunk_from_layer0:{step}.{arg}", set_arg(step, **{arg: ("col", "mod", c[2] - l * cd)})))
        if not fused:
            eps_only.append((f"l{l}.qk_ln_eps_1e-6", set_arg(qstep, ln_eps=1e-6)))
            if fam["prop"] and case.proportional_attn:
                out.append((f"l{l}.self_scale_without_proportional", set_arg(qstep, k_scale=fold(np.float32(math.sqrt(1.0 / hd))))))
        if fam["text"]:
            eps_only.append((f"l{l}.ky_ln_eps_1e-6", set_arg(f"prep.l{l}.ky", ln_eps=1e-6)))
            if case.proportional_attn:
                out.append((f"l{l}.text_scale_with_proportional", set_arg(f"prep.l{l}.ky", out_scale=fold(softmax_scale(case)))))
            out.append((f"l{l}.text_gate_heads_exchanged", set_arg(f"l{l}.attn", tgate=("rows", by[f"l{l}.attn"]["tgate"], [1, 0] + list(range(2, H))))))
    out += moe_mutations(case, by)
    ada = by["adaln.linear"]
    out.append(("final_adaln_bias_dropped", set_arg("adaln.linear", b=("cat", ada["b"][1][:-1] + [zeros(len(fam["final"]) * d)]))))
    out.append(("norm_eps_1e-6", set_everywhere("eps", cfg.norm_eps, 1e-6)))
    # ... and every site that takes norm_eps on its own (the caption y-norm, the first pre-norm, each closing step of a branch: its post-norm
    # and the pre-norm behind it share the operator's one eps argument)
    # (a closing step with neither a post-norm nor an RMS pre-norm behind it - Flag-DiT's last - has no site: the operator does not read eps)
    eps_only += [(f"norm_eps_1e-6@{s.name}", set_arg(s.name, eps=1e-6)) for s in steps if s.args.get("eps") == cfg.norm_eps
                 and (s.op != "grn" or s.args["post_mode"] == 1 or s.args["next_mode"] == 1)]
    last = f"l{L - 1}.grn_ffn"
    eps_only.append(("final_ln_eps_1e-5", set_arg(last, eps_next=1e-5)))
    if "shift" in fam["final"]:
        out.append(("final_shift_scale_exchanged", set_arg(last, next_scale=by[last]["next_shift"], next_shift=by[last]["next_scale"])))
    pm = by["adaln.prep"]
    for i, branch in enumerate(("attn", "ffn")):     # each gate chunk, each scale chunk and the final layer's scale on its own
        if fam["tanh"]:
            out.append((f"gate_without_tanh:{branch}", set_arg("adaln.prep", tanh_mask=pm["tanh_mask"] & ~(1 << fam["gate"][i]))))
        out.append((f"one_plus_scale_as_scale:{branch}", set_arg("adaln.prep", scale_mask=pm["scale_mask"] & ~(1 << fam["scale"][i]))))
    out.append(("one_plus_scale_as_scale:final", set_arg("adaln.prep", final_scale_chunk=-1)))
    out.append(("x_embedder_bias_dropped", set_arg("x_embed", bias=zeros(d))))
    un = by["unpatchify"]
    if case.use_cfg:
        out.append(("cfg_channels_3_4", set_arg("unpatchify", cfg_channels=7 - un["cfg_channels"])))
        if case.B >= 4:      # the uncond row that pairs with cond row i taken from the next sample
            half = case.B // 2
            out.append(("cfg_pairing_shifted", set_arg("unpatchify", sample_perm=list(range(half)) + [half + (i + 1) % half for i in range(half)])))
    if fam["text"]:
        out.append(("cap_embedder_ln_bias_dropped", set_arg("prep.pool", b=zeros(cfg.cap_feat_dim))))
        perm = list(range(case.B))
        perm[0], perm[case.B // 2] = perm[case.B // 2], perm[0]
        out.append(("text_bias_from_other_row", set_arg("prep.bias", mask=("rows", ("in", "mask"), perm))))
    if fam["rope"] == "2d_watershed" and case.scale_factor != 1.0:
        t0 = float(case.inputs["t"][0])
        flipped = 0.0 if t0 < case.scale_watershed else 1.0 + t0
        for l in range(L):
            out.append((f"l{l}.rope_branch_flipped", set_arg(f"l{l}.qkv_post", watershed=flipped)))
    if fam["rope"] != "1d" and case.Hp != case.Wp and not fused:    # token n sits at (n // Wp, n % Wp): the two grid dimensions exchanged
        out.append(("rope_row_col_exchanged", set_arg("l0.qkv_post", grid_w=case.Hp)))
    if fam["eol"]:
        out.append(("eol_token_omitted", drop("eol")))
    if getattr(case, "small_rows", False):
        return eps_only + [m for m in out if m[0] == "norm_eps_1e-6"]     # (the other entries run on the fixtures' own weights)
    return out


def large_mutations(case, steps):
    """[(name, hook)]: one-argument mutations of the steps the large-row regime ADDS (`mutations` covers the steps both lists share).  Names that
    start with "gpu:" change an operand float64 does not model - the transposed table, the partial sums of a projection - so only the GPU
    backend can see them; the "gpu:ystat" entries change words only where the closing step's launcher streams on ystat (Ops.grn_kernels says).
    No entry that is LAUNCHED moves a column block or a buffer's extent: a mutated launch writes exactly where the unmutated one does.  The two
    that would - the qstat width one head short of whole tiles, the V^T split column one head up - are "gpu:refused:" entries: lt_op_qkv_qstat
    refuses them by name (LARGE_REFUSAL) before anything is launched, and the GPU test asserts that refusal."""
    cfg, fam = case.cfg, case.fam
    d, L, hd, H, dkv = cfg.dim, cfg.n_layers, cfg.head_dim, cfg.n_heads, cfg.kv_heads * cfg.head_dim
    by = {s.name: s for s in steps}
    out = []
    two_tables = fam["rope"] == "2d_watershed" and case.scale_factor != 1.0
    if two_tables:
        t0 = float(case.inputs["t"][0])
        flipped = 0.0 if t0 < case.scale_watershed else 1.0 + t0
    plain_scale = fold(np.float32(math.sqrt(1.0 / hd)))
    for l in range(L):
        a = by[f"l{l}.attn"]
        q = by[f"l{l}.qkv"]
        if a.op == "attention_qraw":
            kw, kb = q.args["k_ln_w"], q.args["k_ln_b"]
            out.append((f"l{l}.prologue_q_norm_from_k", set_arg(a.name, q_ln_w=("cat", [kw] * (d // dkv)), q_ln_b=("cat", [kb] * (d // dkv)))))
            out.append((f"l{l}.prologue_q_norm_bias_dropped", set_arg(a.name, q_ln_b=("zeros", d))))
            out.append((f"l{l}.prologue_q_norm_from_other_layer", set_arg(a.name, q_ln_w=by[f"l{(l + 1) % L}.attn"].args["q_ln_w"])))
            if case.Hp != case.Wp:
                out.append((f"l{l}.prologue_grid_w_is_grid_h", set_arg(a.name, grid_w=case.Hp)))
                out.append((f"l{l}.kpass_grid_w_is_grid_h", set_arg(q.name, grid_w=case.Hp)))
            if two_tables:
                out.append((f"l{l}.prologue_watershed_side", set_arg(a.name, watershed=flipped)))
                out.append((f"l{l}.kpass_watershed_side", set_arg(q.name, watershed=flipped)))
                out.append((f"gpu:l{l}.prologue_transposed_table_other_branch", set_arg(a.name, table_t=("flipbr", a.args["table_t"]))))
                out.append((f"l{l}.prologue_table_other_branch", set_arg(a.name, table=("flipbr", a.args["table"]), table_t=("flipbr", a.args["table_t"]))))
            out.append((f"gpu:refused:l{l}.qstat_width_a_head_short_of_whole_tiles", set_arg(q.name, q_cols=d - hd)))
            out.append((f"gpu:refused:l{l}.vt_split_a_head_up", set_arg(q.name, split=d + dkv + hd)))
            if fam["prop"] and case.proportional_attn:
                out.append((f"l{l}.kpass_k_out_scale_without_proportional", set_arg(q.name, k_scale=plain_scale)))
            if fam["text"]:
                out.append((f"l{l}.prologue_text_gate_heads_exchanged", set_arg(a.name, tgate=("rows", a.args["tgate"], [1, 0] + list(range(2, H))))))
                out.append((f"l{l}.prologue_text_keys_from_other_layer", set_arg(a.name, tk=by[f"l{(l + 1) % L}.attn"].args["tk"])))
        p = by.get(f"l{l}.qk_post")
        if p is not None:
            if p.args["q_ln_b"] is not None:
                out.append((f"l{l}.pair_q_norm_bias_dropped", set_arg(p.name, q_ln_b=("zeros", d))))
                out.append((f"l{l}.pair_k_norm_from_other_layer", set_arg(p.name, k_ln_w=by[f"l{(l + 1) % L}.qk_post"].args["k_ln_w"])))
            if fam["prop"] and case.proportional_attn:
                out.append((f"l{l}.pair_k_scale_without_proportional", set_arg(p.name, k_scale=plain_scale)))
            else:
                # (the same product in float64: only the place of the one bf16 rounding the scale is folded into moves)
                out.append((f"gpu:l{l}.pair_q_k_scales_exchanged", set_arg(p.name, q_scale=p.args["k_scale"], k_scale=p.args["q_scale"])))
            if fam["rope"] != "1d" and case.Hp != case.Wp:
                out.append((f"l{l}.pair_grid_w_is_grid_h", set_arg(p.name, grid_w=case.Hp)))
            if two_tables:
                out.append((f"l{l}.pair_watershed_side", set_arg(p.name, watershed=flipped)))
        if f"l{l}.v_vt" in by:     # the V^T launch reading K's rows of the projection weight
            out.append((f"l{l}.vt_from_k_weight", set_arg(f"l{l}.v_vt", w=("w", f"layers.{l}.attention.wk.weight"))))
        if by[f"l{l}.wo"].op == "gemm_ystat":
            ga, gf = by[f"l{l}.grn_attn"].args, by[f"l{l}.grn_ffn"].args
            out.append((f"gpu:ystat:l{l}.grn_ffn:from_the_o_projection", set_arg(f"l{l}.grn_ffn", ystat=ga["ystat"])))
            out.append((f"gpu:ystat:l{l}.grn_attn:from_the_w2_projection_of_the_layer_before" if l else f"gpu:ystat:l{l}.grn_attn:slots_less_a_tile",
                        set_arg(f"l{l}.grn_attn", ystat=by[f"l{l - 1}.grn_ffn"].args["ystat"]) if l else
                        set_arg(f"l{l}.grn_attn", ystat_slots=ga["ystat_slots"] + (-2,))))
            out.append((f"gpu:ystat:l{l}.grn_ffn:slots_less_a_tile", set_arg(f"l{l}.grn_ffn", ystat_slots=gf["ystat_slots"] + (-2,))))
    return out


LARGE_REFUSAL = "lt_op_qkv_qstat: the problem does not take the fused QKV launch with whole Q tiles"
REFUSED_BY_OPERATOR = "fused_router_in_attention_closing_step"     # the float64 chain runs it; lt_op_gated_residual_norm_ex refuses it by name


def moe_mutations(case, by):
    """the wiring mistakes of a mixture-of-experts family, per layer where they are per layer, plus the "layer 1 reads layer 0's" forms"""
    fam, L, out = case.fam, case.cfg.n_layers, []
    moe = fam.get("moe", ())
    if not moe:
        return out
    branches = [br for br, _ in moe]
    both_ = len(moe) == 2
    fused = both_ and "l0.space.route" not in by
    swap = lambda step_a, arg_a, step_b, arg_b: both(set_arg(step_a, **{arg_a: by[step_b][arg_b]}), set_arg(step_b, **{arg_b: by[step_a][arg_a]}))
    tgates = list(by["t.router"]["w"][1]) if "t.router" in by else None
    tgate_set = lambda l, ref: set_arg("t.router", w=("cat", tgates[:l] + [ref] + tgates[l + 1:]))
    # where layer l's space router takes its weight and its input: a step of its own, or the grn step that closes the time branch
    srouter = lambda l: (f"l{l}.grn_time", "route_w") if fused else (f"l{l}.space.route", "gate_w")
    for l in range(L):
        if both_:
            out.append((f"l{l}.time_space_expert_weights_exchanged", both(swap(f"l{l}.time.w13", "w", f"l{l}.space.w13", "w"),
                                                                           swap(f"l{l}.time.w2", "w", f"l{l}.space.w2", "w"))))
            step, arg = srouter(l)      # (both routers are [E, 384] at this size: min(dim, 1024) = dim)
            out.append((f"l{l}.time_space_router_weights_exchanged", both(tgate_set(l, by[step][arg]), set_arg(step, **{arg: tgates[l]}))))
            out.append((f"l{l}.ffn_norms_time_space_exchanged", swap(f"l{l}.grn_time", "post_w", f"l{l}.grn_ffn", "post_w")))
            out.append((f"l{l}.ffn_branch_chunks_exchanged", both(swap(f"l{l}.grn_attn", "next_scale", f"l{l}.grn_time", "next_scale"),
                                                                  swap(f"l{l}.grn_time", "gate", f"l{l}.grn_ffn", "gate"))))
            out.append((f"l{l}.space_combined_through_time_plan", set_arg(f"l{l}.grn_ffn", moe_pos=by[f"l{l}.grn_time"]["moe_pos"],
                                                                          moe_wts=by[f"l{l}.grn_time"]["moe_wts"])))
            if fused:     # the router run by the attention branch's closing step: it routes the TIME branch's input instead of the space branch's
                r = {k: v for k, v in by[f"l{l}.grn_time"].items() if k.startswith("route_")}
                out.append((f"l{l}.fused_router_in_attention_closing_step", both(_add_args(f"l{l}.grn_attn", r), _del_args(f"l{l}.grn_time", list(r)))))
        for br in branches:
            nm = f"l{l}.{br}"
            closing = f"l{l}.grn_time" if (both_ and br == "time") else f"l{l}.grn_ffn"
            pairs = by[f"{nm}.w13"]["w"][1]
            ex = [pairs[e ^ 1] for e in range(len(pairs))]      # experts (0, 1), (2, 3), ... exchanged - whichever of them the fixture uses
            out.append((f"{nm}.experts_exchanged_in_w13_not_w2", set_arg(f"{nm}.w13", w=("experts13", ex))))
            out.append((f"{nm}.w1_w3_exchanged_in_packing", set_arg(f"{nm}.w13", w=("experts13", [(b_, a_) for a_, b_ in pairs]))))
            out.append((f"{nm}.combine_weights_exchanged", set_arg(closing, moe_wts=("swap2", by[closing]["moe_wts"]))))
            if br == "time":
                if len(set(case.inputs["t"].tolist())) > 1:        # (samples that share t share every time-routed choice)
                    lg = by[f"{nm}.plan"]["logits"]
                    out.append((f"{nm}.rows_per_sample_halved", set_arg(f"{nm}.plan", rows_per_sample=case.N // 2, logits=("cat", [lg, lg]))))
            elif not fused:
                out.append((f"{nm}.router_fed_residual_stream", set_arg(f"{nm}.route", x=("buf", "x"))))
            if l > 0:
                if br == "time":
                    out.append((f"{nm}.logits_at_layer0_columns", set_arg(f"{nm}.plan", col0=0)))
                    out.append((f"{nm}.router_weight_from_layer0", tgate_set(l, tgates[0])))
                else:
                    step, arg = srouter(l)
                    out.append((f"{nm}.router_weight_from_layer0", set_arg(step, **{arg: by[srouter(0)[0]][arg]})))
                out.append((f"{nm}.expert_stack_from_layer0", both(set_arg(f"{nm}.w13", w=by[f"l0.{br}.w13"]["w"]), set_arg(f"{nm}.w2", w=by[f"l0.{br}.w2"]["w"]))))
    if tgates:
        out.append(("time_router_fed_adaln_in", set_arg("t.router", a=("buf", "adaln_in"))))
    return out


def _add_args(step, new):
    """hook: arguments the step did not have"""
    def hook(name, args):
        if name == step:
            assert not any(k in args for k in new), (step, list(new))
            args.update(new)
        return args
    return hook


def _del_args(step, names):
    def hook(name, args):
        if name == step:
            for k in names:
                del args[k]
        return args
    return hook


# ---- backend 1: float64 on the CPU ----------------------------------------------------------------------------------------------------------------
class Torch64:
    """every operator in float64, no rounding: buffers are float64 tensors in their logical layout (q / k / v: [B, heads, N, hd])"""

    def __init__(self, case):
        self.case, self.b = case, {}
        self.sel, self.logits = {}, {}      # per sel buffer name ("sel.l0.time", ...): int64 [rows, 2] ascending ids, and the float64 logits they came from

    def ref(self, r):
        if r is None:
            return None
        kind = r[0]
        if kind == "buf":
            return self.b[r[1]]
        if kind == "experts13":
            return [(self.ref(a), self.ref(b)) for a, b in r[1]]
        if kind == "swap2":
            return self.ref(r[1]).reshape(-1, 2).flip(1)
        if kind == "forced":
            return torch.from_numpy(self.case.forced[r[1], r[2]]).long()
        if kind == "flipbr":
            return None if self.ref(r[1]) is None else self.ref(r[1]).flip(0)
        if kind == "slots":
            return None
        if kind == "in":
            v = self.case.inputs[r[1]]
            return v.double() if v.is_floating_point() else v
        if kind == "w":
            return self.case.sd[r[1]].double()
        if kind == "zeros":
            return torch.zeros(r[1], dtype=torch.float64)
        if kind == "cat":
            return torch.cat([self.ref(x) for x in r[1]], 0)
        if kind == "w13":
            return (self.ref(r[1]), self.ref(r[2]))
        if kind == "padk":
            v = self.ref(r[1])
            return torch.cat([v, torch.zeros(v.shape[0], r[2] - v.shape[1], dtype=torch.float64)], 1)
        if kind == "rows":
            return self.ref(r[1])[torch.tensor(r[2])]
        if kind == "col":
            return self.b[r[1]][:, r[2]:r[2] + self.case.cfg.dim]
        raise KeyError(kind)

    def result(self):
        return self.b["out"]

    def op_cast(self, src, dst, n):
        self.b[dst] = self.ref(src).reshape(-1)[:n].clone()

    def op_mask_to_bias(self, mask, dst, B, T, Tpad):
        m = self.ref(mask)
        bias = torch.full((B, Tpad), float("-inf"), dtype=torch.float64)
        bias[:, :T][m != 0] = 0.0
        self.b[dst] = bias

    def op_cap_pool_ln(self, cap, mask, w, b, dst, B, T, C):
        x, m = self.ref(cap).view(B, T, C), self.ref(mask).double()
        pooled = (x * m[:, :, None]).sum(1) / m.sum(1, keepdim=True)
        mean, rstd, _ = R.ln_stats(pooled, 1e-5)
        self.b[dst] = (pooled - mean) * rstd * self.ref(w) + self.ref(b)

    def op_linear(self, a, w, b, dst, M, N, K, act):
        x = self.ref(a).view(M, K)
        if act:
            x = x * torch.sigmoid(x)
        y = x @ self.ref(w).t()
        self.b[dst] = y if b is None else y + self.ref(b)

    # -- mixture of experts: unrounded logits, top-2 with the lowest index winning, softmax over the two, experts combined in ascending id ------
    def _top2(self, logits, forced, sel, wts):
        """logits float64 [rows, E] -> sel [rows, 2] ascending ids, wts [rows, 2] aligned (a forced table replaces the choice, not the weights)"""
        i1 = logits.argmax(1)           # (torch.argmax returns the first maximum on the CPU for float64; ties are checked by the tests' margin)
        rest = logits.clone()
        rest[torch.arange(logits.shape[0]), i1] = float("-inf")
        i2 = rest.argmax(1)
        pick = torch.stack([i1, i2], 1) if forced is None else self.ref(forced)
        pick = pick.sort(1).values
        lg = torch.gather(logits, 1, pick)
        self.b[sel], self.b[wts] = pick, torch.softmax(lg, 1)
        self.sel[sel], self.logits[sel] = pick, logits

    def op_moe_route(self, x, gate_w, forced, rows, rows_per_sample, d, E, max_tiles, sel, wts):
        self._top2(self.ref(x).view(rows, d) @ self.ref(gate_w).t(), forced, sel, wts)

    def op_moe_plan(self, logits, sample_ld, col0, sel_in, forced, rows, rows_per_sample, E, max_tiles, sel, wts, pos, src, te):
        from oracle import moe_plan_oracle as MP
        if logits is not None:
            lg = self.ref(logits).reshape(-1, sample_ld)[:, col0:col0 + E]
            self._top2(lg[torch.arange(rows) // rows_per_sample], forced, sel, wts)
        p, s, t_ = MP.plan(self.b[sel].numpy().astype(np.int32), E, max_tiles)
        self.b[pos], self.b[src], self.b[te] = torch.from_numpy(p).long(), torch.from_numpy(s).long(), torch.from_numpy(t_).long()

    def _grouped(self, a, te, fn, cols):
        out = torch.zeros(a.shape[0], cols, dtype=torch.float64)
        for t_, e in enumerate(te.tolist()):
            if e >= 0:
                out[256 * t_:256 * t_ + 256] = fn(e, a[256 * t_:256 * t_ + 256])
        return out

    def op_gemm_grouped_gather(self, a, a_rows, src, te, w, E, dst, M, N, K):
        x, s, ws = self.ref(a).view(a_rows, K), self.ref(src), self.ref(w)
        g = torch.zeros(M, K, dtype=torch.float64)
        g[s >= 0] = x[s[s >= 0]]

        def swiglu(e, rows):
            a1, a3 = rows @ ws[e][0].t(), rows @ ws[e][1].t()
            return a1 * torch.sigmoid(a1) * a3
        self.b[dst] = self._grouped(g, self.ref(te), swiglu, N // 2)

    def op_gemm_grouped(self, a, te, w, E, dst, M, N, K):
        ws = self.ref(w).view(E, N, K)
        self.b[dst] = self._grouped(self.ref(a).view(M, K), self.ref(te), lambda e, rows: rows @ ws[e].t(), N)

    def op_rmsnorm_mod(self, x, w, scale, shift, dst, B, N, d, eps, ld_mod, scale_pre=0):
        v = self.ref(x).view(B * N, d)
        v = v * R.rms_rinv(v, eps)
        if w is not None:
            v = v * self.ref(w)
        if scale is not None:
            s = self.ref(scale)
            v = v * (s if scale_pre else 1.0 + s).repeat_interleave(N, 0)
        if shift is not None:
            v = v + self.ref(shift).repeat_interleave(N, 0)
        self.b[dst] = v

    def op_gemm(self, a, w, bias, dst, M, N, K, epi, splitk):
        x, wt = self.ref(a).view(M, K), self.ref(w)
        if epi == 1:
            a1, a3 = x @ wt[0].t(), x @ wt[1].t()
            self.b[dst] = a1 * torch.sigmoid(a1) * a3
            return
        y = x @ wt.t()
        self.b[dst] = y if bias is None else y + self.ref(bias)

    def _ln(self, x, w, b, eps):
        if w is None:
            return x
        mean, rstd, _ = R.ln_stats(x, eps)
        return (x - mean) * rstd * self.ref(w) + self.ref(b)

    def op_qk_norm(self, src, ld, col0, ln_w, ln_b, ln_eps, dst, B, N, heads, hd, out_scale):
        x = self._ln(self.ref(src).view(B * N, ld)[:, col0:col0 + heads * hd], ln_w, ln_b, ln_eps) * R.f32(out_scale)
        self.b[dst] = x.view(B, N, heads, hd).permute(0, 2, 1, 3)

    def op_v_transpose(self, src, ld, col0, dst, B, N, Npad, kvh, hd):
        self.b[dst] = self.ref(src).view(B * N, ld)[:, col0:col0 + kvh * hd].view(B, N, kvh, hd).permute(0, 2, 1, 3)

    def op_label_gather(self, table, labels, dst, B, rows, d):
        self.b[dst] = self.ref(table)[self.ref(labels).long().clamp(0, rows - 1)]

    def op_patchify(self, x, dst, B, C, H, W, patch, kpad, dup, wp_stride):
        v = self.ref(x)
        if dup:
            v = torch.cat([v[:B // 2], v[:B // 2]], 0)
        Hp, Wp = H // patch, W // patch
        rows = v.view(B, C, Hp, patch, Wp, patch).permute(0, 2, 4, 1, 3, 5).reshape(B, Hp, Wp, C * patch * patch)
        out = torch.zeros(B, Hp, wp_stride or Wp, kpad, dtype=torch.float64)
        out[:, :, :Wp, :C * patch * patch] = rows
        self.b[dst] = out.view(-1, kpad)

    def op_eol_fill(self, x, eol, rows_total, Wp, d):
        self.b[x].view(rows_total, Wp + 1, d)[:, Wp, :] = self.ref(eol)

    def op_timestep_features(self, t, dst, B, dim):
        self.b[dst] = M.ref_timestep_features(self.ref(t).float(), dim)[0]

    def op_add(self, a, b, dst, n):
        self.b[dst] = self.ref(a) + self.ref(b)

    def op_prep_mod(self, mod, B, ld_mod, L, chunks, d, tanh_mask, scale_mask, final_scale_chunk):
        m = self.b[mod]
        for l in range(L):
            for c in range(chunks):
                v = m[:, (l * chunks + c) * d:(l * chunks + c + 1) * d]
                if tanh_mask >> c & 1:
                    v.copy_(torch.tanh(v))
                if scale_mask >> c & 1:
                    v.copy_(1.0 + v)
        if final_scale_chunk >= 0:
            v = m[:, (L * chunks + final_scale_chunk) * d:(L * chunks + final_scale_chunk + 1) * d]
            v.copy_(1.0 + v)

    def op_rope_table(self, dst, len, hd, step, theta0, lin0, theta1, lin1, lin_on_pos, dst_t=None):
        self.b[dst] = M.ref_rope_table(len, hd, step, theta0, lin0, theta1, lin1, lin_on_pos)[0]
        if dst_t:        # (the transposed copy the attention prologue reads: the same numbers, float64 reads `table` alone)
            self.b[dst_t] = self.b[dst]

    def _branch(self, t, watershed):
        return 1 if t is None or not float(self.ref(t)[0]) < R.f32(watershed) else 0

    def _rope(self, x, B, N, heads, hd, table, rope_mode, branch, grid_w, scale):
        cos, sin = R.rope_factors(self.ref(table), branch, B, N, hd, rope_mode, grid_w)
        v = x.reshape(B * N, heads, hd // 2, 2)
        a0, a1, cos, sin = v[..., 0], v[..., 1], cos[:, None, :], sin[:, None, :]
        v = torch.stack([a0 * cos - a1 * sin, a0 * sin + a1 * cos], -1) * R.f32(scale)
        return v.view(B, N, heads, hd).permute(0, 2, 1, 3)

    def op_qkv_post(self, qkv, ld, q_col0, k_col0, v_col0, q_ln_w, q_ln_b, k_ln_w, k_ln_b, ln_eps, q, k, vt, B, N, Npad, H, Hkv, hd, table, q_scale,
                    k_scale, rope_mode, t, watershed, grid_w, cs_len):
        src, br = self.ref(qkv).view(B * N, ld), self._branch(t, watershed)
        self.b[q] = self._rope(self._ln(src[:, q_col0:q_col0 + H * hd], q_ln_w, q_ln_b, ln_eps), B, N, H, hd, table, rope_mode, br, grid_w, q_scale)
        self.b[k] = self._rope(self._ln(src[:, k_col0:k_col0 + Hkv * hd], k_ln_w, k_ln_b, ln_eps), B, N, Hkv, hd, table, rope_mode, br, grid_w, k_scale)
        self.b[vt] = src[:, v_col0:v_col0 + Hkv * hd].view(B, N, Hkv, hd).permute(0, 2, 1, 3)

    # -- the large-row launches: the float64 meaning of the steps they replace (the qstat / ystat partial sums are not modelled) ----------------
    def op_gemm_qkv(self, a, w, qkv, vt, M, N, K, split, tokens, hd):
        self.op_gemm(a, w, None, qkv, M, N, K, 0, False)
        self.b[vt] = self.b[qkv][:, split:].view(M // tokens, tokens, (N - split) // hd, hd).permute(0, 2, 1, 3)

    def op_qkv_qstat(self, a, w, qkv, vt, M, N, K, split, tokens, hd, q_cols, k_ln_w, k_ln_b, table, t, watershed, grid_w, k_scale, k, qmr):
        self.op_gemm_qkv(a, w, qkv, vt, M, N, K, split, tokens, hd)
        B, kvh = M // tokens, (split - q_cols) // hd
        self.b[k] = self._rope(self._ln(self.b[qkv][:, q_cols:split], k_ln_w, k_ln_b, 1e-5), B, tokens, kvh, hd, table, 1, self._branch(t, watershed),
                               grid_w, k_scale)
        self.b[qmr] = None

    def op_gemm_vt(self, a, w, dst, M, N, K, tokens, hd):
        self.b[dst] = (self.ref(a).view(M, K) @ self.ref(w).t()).view(M // tokens, tokens, N // hd, hd).permute(0, 2, 1, 3)

    def op_qk_post_pair(self, qkv, ld, q_col0, k_col0, q_ln_w, q_ln_b, k_ln_w, k_ln_b, ln_eps, q, k, B, N, H, Hkv, hd, table, q_scale, k_scale, rope_mode,
                        t, watershed, grid_w, cs_len):
        src, br = self.ref(qkv).view(B * N, ld), self._branch(t, watershed)
        self.b[q] = self._rope(self._ln(src[:, q_col0:q_col0 + H * hd], q_ln_w, q_ln_b, ln_eps), B, N, H, hd, table, rope_mode, br, grid_w, q_scale)
        self.b[k] = self._rope(self._ln(src[:, k_col0:k_col0 + Hkv * hd], k_ln_w, k_ln_b, ln_eps), B, N, Hkv, hd, table, rope_mode, br, grid_w, k_scale)

    def op_attention_qraw(self, qkv, ld, q_col0, qmr, q_ln_w, q_ln_b, table, table_t, table_len, grid_w, t, watershed, k, vt, tk, tvt, tbias, tgate,
                          T, Tpad, dst, B, H, Hkv, N, Npad, hd):
        src = self.ref(qkv).view(B * N, ld)
        self.b["_q"] = self._rope(self._ln(src[:, q_col0:q_col0 + H * hd], q_ln_w, q_ln_b, 1e-5), B, N, H, hd, table, 1, self._branch(t, watershed),
                                  grid_w, 1.0)
        if tk is None:
            self.op_attention(("buf", "_q"), k, vt, dst, B, H, Hkv, N, Npad, hd)
        else:
            self.op_attention_fused(("buf", "_q"), k, vt, tk, tvt, tbias, tgate, dst, B, H, Hkv, N, Npad, T, Tpad, hd)

    def op_gemm_ystat(self, a, w, dst, ystat, M, N, K):
        self.op_gemm(a, w, None, dst, M, N, K, 0, False)
        self.b[ystat] = None

    @staticmethod
    def _attend(q, k, v, bias=None):
        """base-2 softmax attention (exact_prologue.attention64's statement) with an additive key bias"""
        if bias is None:
            return P64.attention64(q, k, v)
        rep = q.shape[1] // k.shape[1]
        kd, vd = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
        s = q @ kd.transpose(2, 3) + bias[:, None, None, :k.shape[2]]
        wgt = torch.exp2(s - s.max(-1, keepdim=True).values)
        return (wgt @ vd) / wgt.sum(-1, keepdim=True)

    def op_attention(self, q, k, vt, dst, B, H, Hkv, N, Npad, hd):
        o = self._attend(self.ref(q), self.ref(k), self.ref(vt))
        self.b[dst] = o.permute(0, 2, 1, 3).reshape(B * N, H * hd)

    def op_attention_fused(self, q, k, vt, tk, tvt, tbias, tgate, dst, B, H, Hkv, N, Npad, T, Tpad, hd):
        qq = self.ref(q)
        o = self._attend(qq, self.ref(k), self.ref(vt))
        ot = self._attend(qq, self.ref(tk), self.ref(tvt), self.ref(tbias))
        o = o + ot * torch.tanh(self.ref(tgate)).view(1, H, 1, 1)
        self.b[dst] = o.permute(0, 2, 1, 3).reshape(B * N, H * hd)

    def op_qkv_attention_small(self, a, w, qkv, M, K, H, Hkv, tokens, hd, q_ln_w, q_ln_b, k_ln_w, k_ln_b, table, table_len, grid_w, k_scale, dst):
        d, dkv, B = H * hd, Hkv * hd, M // tokens
        self.op_gemm(a, w, None, qkv, M, d + 2 * dkv, K, 0, False)
        self.op_qkv_post(("buf", qkv), d + 2 * dkv, 0, d, d + dkv, q_ln_w, q_ln_b, k_ln_w, k_ln_b, 1e-5, "_q", "_k", "_v", B, tokens, tokens, H, Hkv,
                         hd, table, 1.0, k_scale, 1, None, 0.0, grid_w, table_len)
        self.op_attention(("buf", "_q"), ("buf", "_k"), ("buf", "_v"), dst, B, H, Hkv, tokens, tokens, hd)

    def op_grn(self, x, y, post_w, gate, post_mode, next_w, next_scale, next_shift, next_mode, ld_mod, h, B, N, d, eps, eps_next, moe_ys=None,
               moe_pos=None, moe_wts=None, route_w=None, route_E=0, route_sel=None, route_wts=None, route_forced=None, ystat=None, ystat_slots=None):
        xv = self.b[x].view(B * N, d)
        if moe_ys is None:
            yv = self.ref(y).view(B * N, d)
        else:       # the top-2 combine, ascending expert id (= _moe_combine's loop order; in float64 the order does not round)
            ys, ps, wt = self.ref(moe_ys), self.ref(moe_pos).reshape(-1, 2), self.ref(moe_wts).reshape(-1, 2)
            yv = wt[:, 0, None] * ys[ps[:, 0]] + wt[:, 1, None] * ys[ps[:, 1]]
        if route_w is not None:
            assert next_mode == 1
        if post_mode == 1:
            yv = yv * R.rms_rinv(yv, eps) * self.ref(post_w)
        xv = xv + self.ref(gate).repeat_interleave(N, 0) * yv
        self.b[x] = xv
        if next_mode == 1:
            self.op_rmsnorm_mod(("buf", x), next_w, next_scale, next_shift, h, B, N, d, eps, ld_mod, scale_pre=1)
            if route_w is not None:
                self._top2(self.b[h] @ self.ref(route_w).t(), route_forced, route_sel, route_wts)
            return
        mean, rstd, _ = R.ln_stats(xv, eps_next)
        v = (xv - mean) * rstd * self.ref(next_scale).repeat_interleave(N, 0)
        self.b[h] = v if next_shift is None else v + self.ref(next_shift).repeat_interleave(N, 0)

    def op_unpatchify(self, rows, ld, dst, B, C, out_ch, H, W, patch, use_cfg, cfg_scale, cfg_channels, wp_stride, sample_perm):
        r = self.ref(rows).view(B, -1, ld)
        if sample_perm is not None:
            r = r[torch.tensor(sample_perm)]
        x = M.unpatchify_index(r.reshape(-1, ld), B, C, out_ch, H, W, patch, wp_stride)
        if use_cfg:
            half, ch = B // 2, min(cfg_channels, C)
            g = x[half:, :ch] + R.f32(cfg_scale) * (x[:half, :ch] - x[half:, :ch])
            x = x.clone()
            x[:half, :ch], x[half:, :ch] = g, g
        self.b[dst] = x


# ---- backend 2: the operator entry points on the GPU ------------------------------------------------------------------------------------------------
class Ops:
    """every step one lt_op_* launch on buffers this object owns.  Outputs: NaN between guard zones (the patch rows are zero-filled instead: the
    patchify contract leaves the eol slots of Flag-DiT unwritten, lumina_dit_debug.h, and the embedder reads every row).  `finish()` checks every guard."""

    def __init__(self, case):
        from gpu_util import P, lib, ok, stream
        self.case, self.P, self.L, self.ok, self.stream = case, P, lib(), ok, stream
        self.g, self.b, self.keep, self.cache = {}, {}, [], {}
        self.slots, self.grn_kernels, self.step = {}, {}, None     # ystat buffer -> slots its launch filled; closing step on ystat -> its row kernel's name
        self.kernels = {}     # grouped GEMM steps: (M, N, K, epilogue) -> the kernel's name (lt_op_gemm_describe; see _grouped_kernel)
        self.part = torch.zeros(256 * 2 * 64 * 128, dtype=torch.float32, device="cuda")     # split-K workspace: 256 slots, counters zero
        self.cnt = torch.zeros(256, dtype=torch.int32, device="cuda")

    def new(self, name, shape, dtype=torch.bfloat16, fill=float("nan")):
        n = int(np.prod(shape))
        g = R.GuardedBuf(n, dtype=dtype, fill=fill)
        if name in self.g:
            self.keep.append(self.g[name])      # (a replaced buffer's guards are still checked at the end)
        self.g[name], self.b[name] = g, g.out.view(*shape)
        return self.b[name]

    def finish(self):
        torch.cuda.synchronize()
        for name, g in list(self.g.items()) + [("(replaced)", g) for g in self.keep]:
            g.assert_intact(f"{self.case.name}: buffer {name}")
        assert int(self.cnt.abs().sum()) == 0, "a split-K tile counter was left non-zero"

    def result(self):
        self.finish()
        return self.b["out"]

    def ref(self, r, dtype=torch.bfloat16):
        """-> a device tensor (weights and inputs: converted and packed once per reference)"""
        if r is None:
            return None
        kind = r[0]
        if kind == "buf":
            return self.b[r[1]]
        if kind == "col":
            return self.b[r[1]].view(-1)[r[2]:]
        if kind == "swap2":
            return self.ref(r[1], dtype).reshape(-1, 2).flip(1).contiguous()
        if kind == "flipbr":
            return self.ref(r[1], dtype).flip(0).contiguous()
        key = repr((r, dtype))
        if key not in self.cache:
            self.cache[key] = self._make(r, dtype)
        return self.cache[key]

    def _make(self, r, dtype):
        kind = r[0]
        if kind == "in":
            v = self.case.inputs[r[1]]
            if r[1] == "x":
                return v.to("cuda", self.case.io_dtype).contiguous()
            return v.to("cuda", dtype if v.is_floating_point() and r[1] != "t" else v.dtype).contiguous()
        if kind == "w":
            return self.case.sd[r[1]].to("cuda", dtype).contiguous()
        if kind == "zeros":
            return torch.zeros(r[1], dtype=dtype, device="cuda")
        if kind == "cat":
            return torch.cat([self.ref(x, dtype) for x in r[1]], 0).contiguous()
        if kind == "padk":
            v = self.ref(r[1], dtype)
            return torch.cat([v, torch.zeros(v.shape[0], r[2] - v.shape[1], dtype=dtype, device="cuda")], 1).contiguous()
        if kind == "rows":
            return self.ref(r[1], dtype)[torch.tensor(r[2], device="cuda")].contiguous()
        if kind == "experts13":
            return torch.cat([self.ref(("w13", a, b)) for a, b in r[1]], 0).contiguous()
        if kind == "forced":
            return torch.from_numpy(self.case.forced[r[1], r[2]]).to("cuda", torch.int32).contiguous()
        if kind == "w13":
            w1, w3 = self.ref(r[1]), self.ref(r[2])
            F, K = w1.shape
            out = torch.full((2 * F, K), float("nan"), dtype=torch.bfloat16, device="cuda")
            self.ok(self.L.lt_op_pack_w13(self.P(w1), self.P(w3), self.P(out), F, K, self.stream()), "pack_w13")
            return out
        raise KeyError(kind)

    def op_cast(self, src, dst, n):
        s = self.ref(src)
        self.ok(self.L.lt_op_cast_to_bf16(self.P(s), 1, self.P(self.new(dst, (n,))), n, self.stream()), "cast_to_bf16")

    def op_mask_to_bias(self, mask, dst, B, T, Tpad):
        self.ok(self.L.lt_op_mask_to_bias(self.P(self.ref(mask)), self.P(self.new(dst, (B, Tpad), torch.float32)), B, T, Tpad, self.stream()), "mask_to_bias")

    def op_cap_pool_ln(self, cap, mask, w, b, dst, B, T, C):
        self.ok(self.L.lt_op_cap_pool_ln(self.P(self.ref(cap)), 1, self.P(self.ref(mask)), self.P(self.ref(w)), self.P(self.ref(b)),
                                         self.P(self.new(dst, (B, C))), B, T, C, self.stream()), "cap_pool_ln")

    def op_linear(self, a, w, b, dst, M, N, K, act):
        self.ok(self.L.lt_op_linear_small_m(self.P(self.ref(a)), self.P(self.ref(w)), self.P(self.ref(b)), self.P(self.new(dst, (M, N))), M, N, K, act,
                                            self.stream()), "linear_small_m")

    def op_rmsnorm_mod(self, x, w, scale, shift, dst, B, N, d, eps, ld_mod, scale_pre=0):
        self.ok(self.L.lt_op_rmsnorm_mod(self.P(self.ref(x)), self.P(self.ref(w)), self.P(self.ref(scale)), self.P(self.ref(shift)), ld_mod,
                                         self.P(self.new(dst, (B * N, d))), B, N, d, eps, scale_pre, self.stream()), "rmsnorm_mod")

    def op_gemm(self, a, w, bias, dst, M, N, K, epi, splitk):
        A, Wt, out = self.ref(a), self.ref(w), self.new(dst, (M, N // 2 if epi == 1 else N))
        if splitk and bias is None and epi == 0:     # the launcher's own decision, with the workspace the engine lends it (lumina_dit.h)
            self.ok(self.L.lt_op_gemm_splitk_auto(self.P(A), self.P(Wt), self.P(out), M, N, K, self.P(self.part), self.P(self.cnt), 256, self.stream()),
                    "gemm_splitk_auto")
        else:
            self.ok(self.L.lt_op_gemm_bf16(self.P(A), self.P(Wt), self.P(self.ref(bias)), 1, self.P(out), M, N, K, epi, 0, self.stream()), "gemm_bf16")

    def op_qk_norm(self, src, ld, col0, ln_w, ln_b, ln_eps, dst, B, N, heads, hd, out_scale):
        self.ok(self.L.lt_op_qk_norm_rope(self.P(self.ref(src)), ld, col0, self.P(self.ref(ln_w)), self.P(self.ref(ln_b)), ln_eps,
                                          self.P(self.new(dst, (B, heads, N, hd))), B, N, heads, hd, 0, self.P(None), 1, out_scale, self.stream()), "qk_norm_rope")

    def op_v_transpose(self, src, ld, col0, dst, B, N, Npad, kvh, hd):
        self.ok(self.L.lt_op_v_transpose(self.P(self.ref(src)), ld, col0, self.P(self.new(dst, (B, kvh, hd, Npad))), B, N, Npad, kvh, hd, self.stream()),
                "v_transpose")

    def op_label_gather(self, table, labels, dst, B, rows, d):
        self.ok(self.L.lt_op_label_gather(self.P(self.ref(table)), self.P(self.ref(labels)), self.P(self.new(dst, (B, d))), B, rows, d, self.stream()),
                "label_gather")

    def op_patchify(self, x, dst, B, C, H, W, patch, kpad, dup, wp_stride):
        xs = self.ref(x)
        rows = B * (H // patch) * (wp_stride or W // patch)
        self.ok(self.L.lt_op_patchify(self.P(xs), 1 if xs.dtype == torch.bfloat16 else 0, self.P(self.new(dst, (rows, kpad), fill=0.0)), B, C, H, W, patch,
                                      kpad, dup, wp_stride, self.stream()), "patchify")

    def op_eol_fill(self, x, eol, rows_total, Wp, d):
        self.ok(self.L.lt_op_eol_fill(self.P(self.b[x]), self.P(self.ref(eol)), rows_total, Wp, d, self.stream()), "eol_fill")

    def op_timestep_features(self, t, dst, B, dim):
        self.ok(self.L.lt_op_timestep_features(self.P(self.ref(t)), 0, self.P(self.new(dst, (B, dim))), B, dim, self.stream()), "timestep_features")

    def op_add(self, a, b, dst, n):
        self.ok(self.L.lt_op_add_bf16(self.P(self.ref(a)), self.P(self.ref(b)), self.P(self.new(dst, (n,))), n, self.stream()), "add_bf16")

    def op_prep_mod(self, mod, B, ld_mod, L, chunks, d, tanh_mask, scale_mask, final_scale_chunk):
        self.ok(self.L.lt_op_prep_mod(self.P(self.b[mod]), B, ld_mod, L, chunks, d, tanh_mask, scale_mask, final_scale_chunk, self.stream()), "prep_mod")

    def op_rope_table(self, dst, len, hd, step, theta0, lin0, theta1, lin1, lin_on_pos, dst_t=None):
        out = self.new(dst, (2, len, hd // step, 2), torch.float32)
        out_t = self.new(dst_t, (2, hd // step, len, 2), torch.float32) if dst_t else None
        self.ok(self.L.lt_op_rope_table(self.P(out), len, hd, step, theta0, lin0, theta1, lin1, lin_on_pos, self.stream(), self.P(out_t)), "rope_table")

    def op_qkv_post(self, qkv, ld, q_col0, k_col0, v_col0, q_ln_w, q_ln_b, k_ln_w, k_ln_b, ln_eps, q, k, vt, B, N, Npad, H, Hkv, hd, table, q_scale,
                    k_scale, rope_mode, t, watershed, grid_w, cs_len):
        f = lambda r: self.P(self.ref(r))
        tt = None if t is None else self.ref(t)
        self.ok(self.L.lt_op_qkv_post(f(qkv), ld, q_col0, k_col0, v_col0, f(q_ln_w), f(q_ln_b), f(k_ln_w), f(k_ln_b), ln_eps,
                                      self.P(self.new(q, (B, H, N, hd))), self.P(self.new(k, (B, Hkv, N, hd))), self.P(self.new(vt, (B, Hkv, hd, Npad))),
                                      B, N, Npad, H, Hkv, hd, rope_mode, f(table), cs_len, self.P(tt), watershed, grid_w, self.P(None), self.P(None),
                                      q_scale, k_scale, self.stream()), "qkv_post")

    def op_attention(self, q, k, vt, dst, B, H, Hkv, N, Npad, hd):
        f = lambda r: self.P(self.ref(r))
        self.ok(self.L.lt_op_attention(f(q), f(k), f(vt), self.P(None), self.P(self.new(dst, (B * N, H * hd))), self.P(None), 0, B, H, Hkv, N, N, Npad, hd,
                                       1.0, 1, self.stream()), "attention")

    def op_attention_fused(self, q, k, vt, tk, tvt, tbias, tgate, dst, B, H, Hkv, N, Npad, T, Tpad, hd):
        f = lambda r: self.P(self.ref(r))
        self.ok(self.L.lt_op_attention_fused(f(q), f(k), f(vt), f(tk), f(tvt), f(tbias), f(tgate), self.P(self.new(dst, (B * N, H * hd))), B, H, Hkv, N, N,
                                             Npad, T, Tpad, hd, self.stream()), "attention_fused")

    def op_qkv_attention_small(self, a, w, qkv, M, K, H, Hkv, tokens, hd, q_ln_w, q_ln_b, k_ln_w, k_ln_b, table, table_len, grid_w, k_scale, dst):
        f = lambda r: self.P(self.ref(r))
        n = H * hd + 2 * Hkv * hd
        ws = self.new("rowstat", (M, (n + 127) // 128, 2), torch.float32)
        self.ok(self.L.lt_op_qkv_attention_small(f(a), f(w), self.P(self.new(qkv, (M, n))), M, K, H, Hkv, tokens, hd, f(q_ln_w), f(q_ln_b), f(k_ln_w), f(k_ln_b),
                                                 f(table), table_len, grid_w, k_scale, self.P(ws), self.P(self.new(dst, (M, H * hd))), self.stream()),
                "qkv_attention_small")

    # -- the large-row launches -----------------------------------------------------------------------------------------------------------------
    def _host_branch(self, t, watershed):
        """the table branch an entry that takes ONE branch's table is handed: 0 when t[0] < watershed (fp32), else - and without t - 1"""
        return 1 if t is None or not float(np.float32(self.case.inputs[t[1]][0])) < float(np.float32(watershed)) else 0

    def op_gemm_qkv(self, a, w, qkv, vt, M, N, K, split, tokens, hd):
        out = self.new(qkv, (M, N))       # (the V columns stay NaN: the launch leaves them untouched and nothing may read them)
        v = self.new(vt, (M // tokens, (N - split) // hd, hd, tokens))
        self.ok(self.L.lt_op_gemm_qkv(self.P(self.ref(a)), self.P(self.ref(w)), self.P(out), self.P(v), M, N, K, split, tokens, hd, self.stream()), "gemm_qkv")

    def op_qkv_qstat(self, a, w, qkv, vt, M, N, K, split, tokens, hd, q_cols, k_ln_w, k_ln_b, table, t, watershed, grid_w, k_scale, k, qmr):
        assert t is None or t[0] == "in"
        f = lambda r: self.P(self.ref(r))
        out, v = self.new(qkv, (M, N)), self.new(vt, (M // tokens, (N - split) // hd, hd, tokens))
        kk = self.new(k, (M // tokens, (split - q_cols) // hd, tokens, hd))
        ws, mr = self.new("qstat", (M, 32, 2), torch.float32), self.new(qmr, (M, 2), torch.float32)
        tab = self.ref(table)[self._host_branch(t, watershed)]
        assert tab.is_contiguous()
        self.ok(self.L.lt_op_qkv_qstat(f(a), f(w), self.P(out), self.P(v), M, N, K, split, tokens, hd, q_cols, f(k_ln_w), f(k_ln_b), self.P(tab), grid_w,
                                       k_scale, self.P(kk), self.P(ws), self.P(mr), self.stream()), "qkv_qstat")

    def op_gemm_vt(self, a, w, dst, M, N, K, tokens, hd):
        v = self.new(dst, (M // tokens, N // hd, hd, tokens))
        self.ok(self.L.lt_op_gemm_vt(self.P(self.ref(a)), self.P(self.ref(w)), self.P(v), M, N, K, tokens, hd, 0, self.stream()), "gemm_vt")

    def op_qk_post_pair(self, qkv, ld, q_col0, k_col0, q_ln_w, q_ln_b, k_ln_w, k_ln_b, ln_eps, q, k, B, N, H, Hkv, hd, table, q_scale, k_scale, rope_mode,
                        t, watershed, grid_w, cs_len):
        f = lambda r: self.P(self.ref(r))
        tt = None if t is None else self.ref(t)
        self.ok(self.L.lt_op_qk_norm_rope_pair(f(qkv), ld, q_col0, k_col0, f(q_ln_w), f(q_ln_b), f(k_ln_w), f(k_ln_b), ln_eps, self.P(self.new(q, (B, H, N, hd))),
                                               self.P(self.new(k, (B, Hkv, N, hd))), B, N, H, Hkv, hd, rope_mode, f(table), cs_len, self.P(tt), watershed,
                                               grid_w, self.P(None), self.P(None), q_scale, k_scale, self.stream()), "qk_norm_rope_pair")

    def op_attention_qraw(self, qkv, ld, q_col0, qmr, q_ln_w, q_ln_b, table, table_t, table_len, grid_w, t, watershed, k, vt, tk, tvt, tbias, tgate,
                          T, Tpad, dst, B, H, Hkv, N, Npad, hd):
        f = lambda r: self.P(self.ref(r))
        tt = None if t is None else self.ref(t)
        self.ok(self.L.lt_op_attention_qraw_ex(f(qkv), ld, q_col0, f(qmr), f(q_ln_w), f(q_ln_b), f(table), f(table_t), table_len, grid_w, self.P(tt),
                                               watershed, f(k), f(vt), f(tk), f(tvt), f(tbias), f(tgate), T, Tpad, self.P(self.new(dst, (B * N, H * hd))),
                                               B, H, Hkv, N, Npad, hd, self.stream()), "attention_qraw_ex")

    def op_gemm_ystat(self, a, w, dst, ystat, M, N, K):
        cap = 2 * (-(-N // 256))
        ws, n = self.new(ystat, (M, cap), torch.float32), ctypes.c_int32(0)
        self.ok(self.L.lt_op_gemm_ystat(self.P(self.ref(a)), self.P(self.ref(w)), self.P(self.new(dst, (M, N))), self.P(ws), cap, M, N, K, ctypes.byref(n),
                                        self.stream()), "gemm_ystat")
        assert 0 < n.value <= cap and n.value % 2 == 0, (ystat, n.value, cap)
        self.slots[ystat] = n.value

    # -- mixture of experts --------------------------------------------------------------------------------------------------------------------
    def _plan_bufs(self, rows, sel, wts):
        """sel / wts of a router: int32 / bf16 [rows][2] with the 4 words of slack the plan kernel's 16-byte accesses may touch (lumina_dit.h)"""
        return self.new(sel, (2 * rows + 4,), torch.int32, fill=-1), self.new(wts, (2 * rows + 4,), fill=0.0)

    def op_moe_route(self, x, gate_w, forced, rows, rows_per_sample, d, E, max_tiles, sel, wts):
        s, w_ = self._plan_bufs(rows, sel, wts)
        self.ok(self.L.lt_op_moe_route(self.P(self.ref(x)), self.P(self.ref(gate_w)), self.P(self.ref(forced)), rows, rows_per_sample, d, E, self.P(s), self.P(w_),
                                       max_tiles, self.stream()), "moe_route")

    def op_moe_plan(self, logits, sample_ld, col0, sel_in, forced, rows, rows_per_sample, E, max_tiles, sel, wts, pos, src, te):
        if logits is not None:
            s, w_ = self._plan_bufs(rows, sel, wts)
            lp = ctypes.c_void_p(self.ref(logits).data_ptr() + 2 * col0)
        else:
            s, w_, lp = self.ref(sel_in), None, self.P(None)
        p_ = self.new(pos, (2 * rows + 4,), torch.int32, fill=-1)
        self.ok(self.L.lt_op_moe_plan_ex(self.P(s), lp, sample_ld, self.P(self.ref(forced)), self.P(w_), rows, rows_per_sample, E, self.P(p_),
                                         self.P(self.new(src, (max_tiles * 256,), torch.int32, fill=-2)), self.P(self.new(te, (max_tiles,), torch.int32, fill=-2)),
                                         max_tiles, 1, 0, 0, 0, self.stream()), "moe_plan_ex")

    def _grouped_kernel(self, step, M, N, K, epi):
        """variant 0: the launcher chooses as it does for the engine.  A grouped problem goes through the same choose() as a dense one of its
        shape unless the persistent kernel's grouped mode takes it, from 1.5 tiles of 256 x 256 per CU on (gemm_bf16.hip) - asserted not to be
        the case here, so lt_op_gemm_describe names the kernel"""
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert 2 * (M // 256) * (-(-N // 256)) < 3 * cus, ("the persistent grouped kernel would take this problem", M, N, cus)
        buf = ctypes.create_string_buffer(200)
        self.ok(self.L.lt_op_gemm_describe(M, N, K, epi, 0, buf, 200), "gemm_describe")
        self.kernels[step] = buf.value.decode()

    def op_gemm_grouped_gather(self, a, a_rows, src, te, w, E, dst, M, N, K):
        self._grouped_kernel(("w13", M, N, K), M, N, K, 1)
        self.ok(self.L.lt_op_gemm_grouped_gather(self.P(self.ref(a)), a_rows, self.P(self.ref(src)), self.P(self.ref(w)), self.P(self.ref(te)), N * K,
                                                 self.P(self.new(dst, (M, N // 2))), M, N, K, 1, 0, self.stream()), "gemm_grouped_gather")

    def op_gemm_grouped(self, a, te, w, E, dst, M, N, K):
        self._grouped_kernel(("w2", M, N, K), M, N, K, 0)
        self.ok(self.L.lt_op_gemm_grouped(self.P(self.ref(a)), self.P(self.ref(w)), self.P(self.ref(te)), N * K, self.P(self.new(dst, (M, N))), M, N, K, 0, 0,
                                          self.stream()), "gemm_grouped")

    def op_grn(self, x, y, post_w, gate, post_mode, next_w, next_scale, next_shift, next_mode, ld_mod, h, B, N, d, eps, eps_next, moe_ys=None,
               moe_pos=None, moe_wts=None, route_w=None, route_E=0, route_sel=None, route_wts=None, route_forced=None, ystat=None, ystat_slots=None):
        f = lambda r: self.P(self.ref(r))
        if ystat is not None:      # the partial sums the projection left: the launcher streams on them where it has that form, else reduces y itself
            slots = self.slots[ystat_slots[1]] + (ystat_slots[2] if len(ystat_slots) > 2 else 0)
            name = ctypes.create_string_buffer(100)
            self.ok(self.L.lt_op_gated_residual_norm_describe(post_mode, 0, next_mode, d, int(next_w is not None), int(next_scale is not None),
                                                              int(next_shift is not None), 1, 1, slots, 0, name, 100), "gated_residual_norm_describe")
            self.grn_kernels[self.step] = name.value.decode()
            self.ok(self.L.lt_op_gated_residual_norm_ex(self.P(self.b[x]), f(y), f(post_w), f(gate), post_mode, 0, f(next_w), f(next_scale), f(next_shift), next_mode,
                                                        ld_mod, self.P(self.new(h, (B * N, d))), B, N, d, eps, eps_next, 1, 0, f(ystat), slots, self.P(None),
                                                        self.P(None), self.P(None), self.P(None), 0, self.P(None), self.P(None), self.P(None), self.stream()),
                    "gated_residual_norm_ex (ystat)")
            return
        if moe_ys is not None or route_w is not None:
            rs, rw = self._plan_bufs(B * N, route_sel, route_wts) if route_w is not None else (None, None)
            self.ok(self.L.lt_op_gated_residual_norm_ex(self.P(self.b[x]), f(y), f(post_w), f(gate), post_mode, 0, f(next_w), f(next_scale), f(next_shift), next_mode,
                                                        ld_mod, self.P(self.new(h, (B * N, d))), B, N, d, eps, eps_next, 1, 0, self.P(None), 0, f(moe_ys),
                                                        f(moe_pos), f(moe_wts), f(route_w), route_E, self.P(rs), self.P(rw), f(route_forced), self.stream()),
                    "gated_residual_norm_ex")
            return
        self.ok(self.L.lt_op_gated_residual_norm(self.P(self.b[x]), f(y), f(post_w), f(gate), post_mode, 0, f(next_w), f(next_scale), f(next_shift), next_mode,
                                                 ld_mod, self.P(self.new(h, (B * N, d))), B, N, d, eps, eps_next, 1, self.stream()), "gated_residual_norm")

    def op_unpatchify(self, rows, ld, dst, B, C, out_ch, H, W, patch, use_cfg, cfg_scale, cfg_channels, wp_stride, sample_perm):
        r = self.ref(rows)
        if sample_perm is not None:
            r = r.view(B, -1, ld)[torch.tensor(sample_perm, device="cuda")].contiguous()
        dt = self.case.io_dtype
        self.ok(self.L.lt_op_unpatchify_cfg(self.P(r), ld, self.P(self.new(dst, (B, C, H, W), dt)), 1 if dt == torch.bfloat16 else 0, B, C, out_ch, H, W, patch,
                                            use_cfg, cfg_scale, cfg_channels, wp_stride, self.stream()), "unpatchify_cfg")


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the fixtures' cases ------------------------------------------------------------------------------------------------------------------------
GOLDENS = {"next_t2i": ("nextdit_tiny", "nextdit_tiny_rect", "nextdit_tiny_gqa"), "imagenet": ("imagenet_tiny",), "flag_t2i": ("flag_tiny",),
           "moe_time": ("moe_time_tiny",), "moe_space": ("moe_space_tiny",), "moe": ("moe_tiny",)}
MOE_GOLDENS = ("moe_time_tiny", "moe_space_tiny", "moe_tiny")


def load_golden(golden_dir, name):
    import json
    import os

    from oracle import synth
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    return g, cfg, synth.synth_state_dict(cfg, seed=int(g["seed_w"]))


def golden_case(golden_dir, name, mode, **over):
    """mode 'forward': the plain forward as the public classes make it after construction (NTK branch at scale factor 1: watershed 0, no
    proportional attention); 'cfg4': forward_with_cfg at scale 4 with proportional attention against base_seqlen 16 where the family has it;
    'lin2' / 'ntk2' (next_t2i): cfg4 at scale_factor 2, watershed 0.3, t = 0.1 / 0.8 - the two RoPE branches; 'cfg4-t2' (the MoE fixtures, whose
    two samples share t = 0.5 and with it every time-routed choice): cfg4 with t = (0.35, 0.8), so that the samples' time routers differ"""
    g, cfg, sd = load_golden(golden_dir, name)
    x, t = torch.from_numpy(g["z"]), torch.from_numpy(g["t"])
    kw = dict(name=f"{name}-{mode}")
    if cfg.has_text:
        kw.update(cap=torch.from_numpy(g["cap"]), mask=torch.from_numpy(g["mask"]))
    else:
        kw.update(labels=torch.from_numpy(g["y"]))
    if mode == "forward":
        kw.update(use_cfg=False, scale_watershed=0.0)
    else:
        kw.update(use_cfg=True, cfg_scale=4.0)
        if FAMILY[cfg.family]["prop"]:
            kw.update(base_seqlen=16, proportional_attn=True)
        if mode == "cfg4-t2":
            t = torch.tensor([0.35, 0.8])
        if mode in ("lin2", "ntk2"):
            kw.update(scale_factor=2.0, scale_watershed=0.3)
            t = torch.full_like(t, 0.1 if mode == "lin2" else 0.8)
    kw.update(over)
    return Case(cfg, sd, kw.pop("x", x), kw.pop("t", t), **kw)


def oracle_fp32(case, moe_hook=None):
    """the fp32 oracle on the case's (bf16-valued) weights and inputs; guidance on channels [:3] as the reference has it.  moe_hook: a
    variants_oracle.MoeRouting that records (or forces) the experts of every layer and branch"""
    from oracle import nextdit_oracle as O
    from oracle import variants_oracle as V
    i, fam = case.inputs, case.cfg.family
    assert not case.use_cfg or case.cfg_channels == 3
    if fam == "next_t2i":
        kw = dict(proportional_attn=case.proportional_attn, base_seqlen=case.base_seqlen)
        if case.use_cfg:
            return O.forward_with_cfg(case.sd, case.cfg, i["x"], i["t"], i["cap"], i["mask"], case.cfg_scale, scale_factor=case.scale_factor,
                                      scale_watershed=case.scale_watershed, **kw)
        table = O.rope_table(case.cfg.head_dim, 384, scale_factor=case.scale_factor, scale_watershed=case.scale_watershed, timestep=float(i["t"][0]))
        return O.forward(case.sd, case.cfg, i["x"], i["t"], i["cap"], i["mask"], freqs_table=table, **kw)
    if fam in ("imagenet", "moe_time", "moe_space", "moe"):
        if case.use_cfg:
            return V.imagenet_forward_with_cfg(case.sd, case.cfg, i["x"], i["t"], i["labels"].long(), case.cfg_scale, moe_hook=moe_hook)
        return V.imagenet_forward(case.sd, case.cfg, i["x"], i["t"], i["labels"].long(), moe_hook=moe_hook)
    kw = dict(proportional_attn=case.proportional_attn, base_seqlen=case.base_seqlen)
    if case.use_cfg:
        return V.flag_forward_with_cfg(case.sd, case.cfg, i["x"], i["t"], i["cap"], i["mask"], case.cfg_scale, **kw)
    return V.flag_forward(case.sd, case.cfg, i["x"], i["t"], i["cap"], i["mask"], **kw)


def batch6_case(golden_dir, **over):
    """three images (batch 6 = 3 cond + 3 uncond rows) with different latents, timesteps, captions and ragged masks, cfg 4"""
    g, cfg, sd = load_golden(golden_dir, "nextdit_tiny")
    gen = torch.Generator().manual_seed(5)
    n = 3
    zc = torch.randn(n, 4, 16, 16, generator=gen)
    t1 = torch.tensor([0.2, 0.5, 0.9])
    cap = torch.randn(2 * n, 16, cfg.cap_feat_dim, generator=gen)
    mask = torch.ones(2 * n, 16, dtype=torch.int32)
    for i in range(n):
        mask[i, 16 - 2 * i:] = 0
        mask[n + i, 8 - i:] = 0
    kw = dict(cap=cap, mask=mask, use_cfg=True, cfg_scale=4.0, base_seqlen=16, proportional_attn=True, name="nextdit_tiny-batch6")
    kw.update(over)
    return Case(cfg, sd, torch.cat([zc, zc]), torch.cat([t1, t1]), **kw)


def eps_case(golden_dir, name):
    """the golden's cfg-4 call on weights scaled by powers of two (exact in bf16) so that every normalised row has a mean square comparable to
    the eps of its norm: the patch embedder (and eol token) and the adaLN rows of the gate chunks by 2^-9 - the residual stream stays near
    2^-9, where norm_eps 1e-5 and the final LayerNorm's 1e-6 decide the statistic - and wq, wk, wk_y by 2^-8 for the q / k / ky LayerNorms (1e-5), and the caption
    features by 2^-8 for the caption y-norm (norm_eps).  `mutations` returns the eps entries alone for such a case."""
    c0 = golden_case(golden_dir, name, "cfg4")
    sd, d, fam = dict(c0.sd), c0.cfg.dim, c0.fam
    for k in ("x_embedder.weight", "x_embedder.bias", "eol_token"):
        if k in sd:
            sd[k] = sd[k] * 2.0 ** -9
    for l in range(c0.cfg.n_layers):
        for k in ("weight", "bias"):
            m = sd[f"layers.{l}.adaLN_modulation.1.{k}"].clone()
            for g in fam["gate"]:
                m[g * d:(g + 1) * d] *= 2.0 ** -9
            sd[f"layers.{l}.adaLN_modulation.1.{k}"] = m
        for k in ("wq", "wk", "wk_y"):
            key = f"layers.{l}.attention.{k}.weight"
            if key in sd:
                sd[key] = sd[key] * 2.0 ** -8
    i = c0.inputs
    kw = dict(use_cfg=True, cfg_scale=4.0, name=f"{name}-eps")
    if fam["prop"]:
        kw.update(base_seqlen=16, proportional_attn=True)
    if fam["text"]:
        kw.update(cap=i["cap"] * 2.0 ** -8, mask=i["mask"])
    else:
        kw.update(labels=i["labels"])
    c = Case(c0.cfg, sd, i["x"], i["t"], **kw)
    c.small_rows = True
    return c
