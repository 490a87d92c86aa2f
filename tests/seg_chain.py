"""The operator chain of an evaluation with blurred-query blocks (smoothed-energy guidance), on the step list of forward_chain.py.

`seg_steps(case, steps, plain, Q, S, taps, mode)` rewrites the step list of one evaluation (`steps`: the family's default list; `plain`: the
list built with {"small_fused": False}, whose attention steps a blurred block takes): the blocks of S lose their steps (pag_chain.pag_steps
with an empty perturb set), and in the blocks of Q the attention steps become
  "l{l}.qkv"        (plain)        Q | K | V in one plain launch
  "l{l}.qkv_post"   (plain)        q_norm + RoPE on Q -> "q", k_norm + RoPE on K -> "k", V^T -> "vt"
  "l{l}.blur"       query_blur     the post-RoPE queries "q" -> "q_blur" over the token grid (grid_w = the row stride, blur_w = the image columns)
  "l{l}.attn"       attention      self-attention on "q_blur", WITHOUT the text keys
  "l{l}.attn_text"  attention_text (text families) attn += tanh(gate) * softmax(q ky^T + bias) vy on the UNBLURRED "q", accumulate mode
`before_rope=l`: the wiring mistake "blur before RoPE" in block l, as steps of its own (q_norm alone, the blur, then RoPE alone).
`seg_mutations` lists the other wiring mistakes of the issue as hooks."""
import torch

import exact_seg as XS
import forward_chain as FC
import pag_chain as PC

Step = FC.Step
PARTS = ("qkv_attn", "qkv", "qkv_post", "attn")


def seg_steps(case, steps, plain, Q, S, taps, mode, before_rope=None):
    cfg, fam = case.cfg, case.fam
    H, Hkv, hd, B, N = cfg.n_heads, cfg.kv_heads, cfg.head_dim, case.B, case.N
    Q = set(Q)
    assert not (Q & set(S)) and all(0 <= l < cfg.n_layers for l in Q)
    pl = {s.name: s for s in plain}
    grid_w = case.Wrow if fam["eol"] else case.Wp
    out, done = [], set()
    for s in PC.pag_steps(case, steps, (), S):
        l = int(s.name[1:s.name.index(".")]) if s.name[0] == "l" and s.name[1].isdigit() else None
        if l is None or l not in Q or s.name.split(".", 1)[1] not in PARTS:
            out.append(s)
            continue
        if l in done:
            continue
        done.add(l)
        post, at = pl[f"l{l}.qkv_post"], pl[f"l{l}.attn"].args
        out += [pl[f"l{l}.qkv"], post]
        src = "q"
        if before_rope == l:
            a = post.args
            keep = ("ln_eps", "B", "N", "hd", "table", "t", "watershed", "grid_w", "cs_len")
            out.append(Step(f"l{l}.q_norm_only", "q_post", dict(src=a["qkv"], ld=a["ld"], col0=a["q_col0"], ln_w=a["q_ln_w"], ln_b=a["q_ln_b"], dst="qn",
                                                              heads=H, out_scale=a["q_scale"], rope_mode=0, **{k: a[k] for k in keep})))
            src = "qn"
        out.append(Step(f"l{l}.blur", "query_blur", dict(q=("buf", src), dst="q_blur", B=B, H=H, N=N, hd=hd, grid_w=grid_w, blur_w=case.Wp,
                                                         taps=list(taps), mode=mode, reflect=True)))
        if before_rope == l:
            a = post.args
            keep = ("B", "N", "hd", "table", "rope_mode", "t", "watershed", "grid_w", "cs_len")
            out.append(Step(f"l{l}.rope_only", "rope_heads", dict(src=("buf", "q_blur"), dst="q_blur2", heads=H, **{k: a[k] for k in keep})))
        out.append(Step(f"l{l}.attn", "attention", dict(q=("buf", "q_blur2" if before_rope == l else "q_blur"), k=at["k"], vt=at["vt"], dst="attn", B=B, H=H,
                                                        Hkv=Hkv, N=N, Npad=at["Npad"], hd=hd)))
        if fam["text"]:
            out.append(Step(f"l{l}.attn_text", "attention_text", dict(q=("buf", "q"), tk=at["tk"], tvt=at["tvt"], tbias=at["tbias"], tgate=at["tgate"],
                                                                     dst="attn", B=B, H=H, Hkv=Hkv, N=N, T=at["T"], Tpad=at["Tpad"], hd=hd, tanh=True)))
    assert done == Q - set(S)
    return out


class Ops(PC.Ops):
    def op_query_blur(self, q, dst, B, H, N, hd, grid_w, blur_w, taps, mode, reflect):
        src = self.ref(q)
        out = self.new(dst, (B, H, N, hd))
        if not reflect:     # the mutated boundary rule has no kernel: the edge repeated, in float64 on the words, one rounding
            out.copy_(XS.rn_bf16(XS.blur_ref(src.cpu().view(B, H, N, hd), grid_w, blur_w, taps, edge=XS.clamp)).to(torch.bfloat16))
            return
        tp = torch.tensor(taps, dtype=torch.float32, device="cuda") if mode == 0 else None
        self.keep.append(R_keep(tp))
        self.ok(self.L.lt_op_query_blur(self.P(src), self.P(out), self.P(tp), B, H, N, hd, grid_w, blur_w, (len(taps) - 1) // 2 if mode == 0 else 0,
                                        mode, self.stream()), "query_blur")

    def op_rope_heads(self, src, dst, heads, B, N, hd, table, rope_mode, t, watershed, grid_w, cs_len):
        """RoPE alone on a [B, heads, N, hd] buffer: its words as rows [B * N][heads * hd], then the row kernel without a norm"""
        rows = self.new("_rope_rows", (B * N, heads * hd))
        rows.copy_(self.ref(src).view(B, heads, N, hd).permute(0, 2, 1, 3).reshape(B * N, heads * hd))
        self.op_q_post(("buf", "_rope_rows"), heads * hd, 0, None, None, 1e-5, dst, B, N, heads, hd, table, 1.0, rope_mode, t, watershed, grid_w, cs_len)


class R_keep:
    """keeps a tensor alive until the backend finishes (the launch is asynchronous)"""

    def __init__(self, t):
        self.t = t

    def assert_intact(self, what=""):
        pass


def seg_mutations(case, steps, Q, taps_other):
    """[(name, hook)] on the steps of `seg_steps`: each a wiring mistake of one blurred block"""
    cfg, fam = case.cfg, case.fam
    by = {s.name: s.args for s in steps}
    out = []
    for l in sorted(Q):
        at = by[f"l{l}.attn"]
        out.append((f"l{l}.blur_k_instead_of_q", FC.both(FC.set_arg(f"l{l}.blur", q=at["k"], dst="k_blur", H=cfg.kv_heads),
                                                        FC.set_arg(f"l{l}.attn", q=("buf", "q"), k=("buf", "k_blur")))))
        out.append((f"l{l}.wrong_radius", FC.set_arg(f"l{l}.blur", taps=list(taps_other))))
        out.append((f"l{l}.no_reflection", FC.set_arg(f"l{l}.blur", reflect=False)))
        if fam["text"]:
            out.append((f"l{l}.text_on_the_blurred_q", FC.set_arg(f"l{l}.attn_text", q=("buf", "q_blur"))))
    return out
