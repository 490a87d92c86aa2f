"""Perturbed-attention guidance on the operator chain of tests/forward_chain.py (plain module, no test in here; forward_chain is
imported unchanged).

`pag_steps(case, steps, P, S)` rewrites the step list of one evaluation: the blocks of S lose their steps (whoever prepares h prepares it for
the next block that runs), and in the blocks of P the attention step or steps are replaced by
  no text:  "l{l}.v"        gemm             V alone: h x wv^T -> [M][dkv]
            "l{l}.attn_id"  attention_identity   attn[b, n, h, :] = V[b, n, h // (H / Hkv), :]
  text:     "l{l}.qkv"      (kept)           Q | K | V in one launch; K is not read
            "l{l}.q_post"   q_post           q_norm + RoPE on the Q columns -> [B, H, N, hd]
            "l{l}.attn_id"  attention_identity   on the V columns of the QKV buffer
            "l{l}.attn_text" attention_text  attn += tanh(gate) * softmax(q ky^T + bias) vy: the stand-alone text launch, accumulate mode
`Torch64` / `Ops` extend forward_chain's two backends by these three operators.  `EyeTorch64` is the independent restatement: the UNCHANGED
step list in float64, where a perturbed block's self-attention weights are an explicit identity matrix multiplied onto V.
`pag_mutations` lists the wiring mistakes of the issue as hooks on the new steps."""
import numpy as np
import torch

import forward_chain as FC

Step = FC.Step


def pag_steps(case, steps, P, S=()):
    cfg, fam = case.cfg, case.fam
    d, L, H, Hkv, hd = cfg.dim, cfg.n_layers, cfg.n_heads, cfg.kv_heads, cfg.head_dim
    dkv, B, N, M_ = Hkv * hd, case.B, case.N, case.B * case.N
    P, S = set(P), set(S)
    assert not (P & S) and all(0 <= l < L for l in P | S) and len(S) < L
    by = {s.name: s for s in steps}
    layer_of = lambda name: int(name[1:name.index(".")]) if name[0] == "l" and name[1].isdigit() else None
    run = [l for l in range(L) if l not in S]
    nxt = {l: next((m for m in run if m > l), L) for l in range(-1, L)}
    prep = lambda target: by[f"l{target - 1}.grn_ffn"].args      # the closing step that prepares h for layer `target` (L: the final form)
    out = []
    for s in steps:
        l = layer_of(s.name)
        if s.name == "l0.prenorm" and nxt[-1] != 0:          # the first block that runs is not block 0
            a = prep(nxt[-1])
            out.append(Step(s.name, s.op, dict(s.args, w=a["next_w"], scale=a["next_scale"], shift=a["next_shift"])))
            continue
        if l is None or (l not in P and l not in S):
            if l is not None and s.name == f"l{l}.grn_ffn" and nxt[l] != l + 1:
                a = prep(nxt[l])
                s = Step(s.name, s.op, dict(s.args, next_w=a["next_w"], next_scale=a["next_scale"], next_shift=a["next_shift"], next_mode=a["next_mode"]))
            out.append(s)
            continue
        if l in S:
            continue
        p = f"layers.{l}.attention."
        part = s.name.split(".", 1)[1]
        if part == "grn_ffn" and nxt[l] != l + 1:
            a = prep(nxt[l])
            s = Step(s.name, s.op, dict(s.args, next_w=a["next_w"], next_scale=a["next_scale"], next_shift=a["next_shift"], next_mode=a["next_mode"]))
        if part not in ("qkv_attn", "qkv", "qkv_post", "attn"):
            out.append(s)
            continue
        ident = dict(dst="attn", B=B, N=N, H=H, Hkv=Hkv, hd=hd, head_map="div")
        if not fam["text"]:
            if part in ("qkv_attn", "qkv"):
                out.append(Step(f"l{l}.v", "gemm", dict(a=("buf", "h"), w=("w", p + "wv.weight"), bias=None, dst="qkv", M=M_, N=dkv, K=d, epi=0, splitk=True)))
                out.append(Step(f"l{l}.attn_id", "attention_identity", dict(src=("buf", "qkv"), ld=dkv, col0=0, **ident)))
            continue
        if part == "qkv":
            out.append(s)
        elif part == "qkv_post":
            a = s.args
            keep = ("ln_eps", "B", "N", "hd", "table", "rope_mode", "t", "watershed", "grid_w", "cs_len")
            out.append(Step(f"l{l}.q_post", "q_post", dict(src=a["qkv"], ld=a["ld"], col0=a["q_col0"], ln_w=a["q_ln_w"], ln_b=a["q_ln_b"], dst="q",
                                                          heads=H, out_scale=a["q_scale"], **{k: a[k] for k in keep})))
            out.append(Step(f"l{l}.attn_id", "attention_identity", dict(src=a["qkv"], ld=a["ld"], col0=a["v_col0"], **ident)))
        else:
            a = s.args
            out.append(Step(f"l{l}.attn_text", "attention_text", dict(q=a["q"], tk=a["tk"], tvt=a["tvt"], tbias=a["tbias"], tgate=a["tgate"], dst="attn",
                                                                     B=B, H=H, Hkv=Hkv, N=N, T=a["T"], Tpad=a["Tpad"], hd=hd, tanh=True)))
    return out


def head_index(H, Hkv, head_map):
    return [h // (H // Hkv) if head_map == "div" else h % Hkv for h in range(H)]


class Torch64(FC.Torch64):
    def op_attention_identity(self, src, ld, col0, dst, B, N, H, Hkv, hd, head_map):
        v = self.ref(src).view(B * N, ld)[:, col0:col0 + Hkv * hd].view(B * N, Hkv, hd)
        self.b[dst] = v[:, torch.tensor(head_index(H, Hkv, head_map))].reshape(B * N, H * hd).clone()

    def op_q_post(self, src, ld, col0, ln_w, ln_b, ln_eps, dst, B, N, heads, hd, table, out_scale, rope_mode, t, watershed, grid_w, cs_len):
        x = self._ln(self.ref(src).view(B * N, ld)[:, col0:col0 + heads * hd], ln_w, ln_b, ln_eps)
        self.b[dst] = self._rope(x, B, N, heads, hd, table, rope_mode, self._branch(t, watershed), grid_w, out_scale)

    def op_attention_text(self, q, tk, tvt, tbias, tgate, dst, B, H, Hkv, N, T, Tpad, hd, tanh):
        ot = self._attend(self.ref(q), self.ref(tk), self.ref(tvt), self.ref(tbias))
        g = self.ref(tgate)
        ot = ot * (torch.tanh(g) if tanh else g).view(1, H, 1, 1)
        self.b[dst] = self.b[dst] + ot.permute(0, 2, 1, 3).reshape(B * N, H * hd)


class EyeTorch64(FC.Torch64):
    """the unchanged step list; in the blocks of `perturbed` the self-attention weights are the identity matrix (use `hook` with FC.run)"""

    def __init__(self, case, perturbed):
        super().__init__(case)
        self.perturbed, self.eye_now = set(perturbed), False

    def hook(self, name, args):
        self.eye_now = name[0] == "l" and name[1].isdigit() and int(name[1:name.index(".")]) in self.perturbed
        return args

    def _attend(self, q, k, v, bias=None):
        if bias is not None or not self.eye_now:
            return FC.Torch64._attend(q, k, v, bias)
        rep = q.shape[1] // k.shape[1]
        vd = v.repeat_interleave(rep, 1)                                  # [B, H, N, hd]: head h reads kv head h // rep
        wgt = torch.eye(q.shape[2], dtype=torch.float64).expand(q.shape[0], q.shape[1], -1, -1)
        return wgt @ vd


class Ops(FC.Ops):
    def op_attention_identity(self, src, ld, col0, dst, B, N, H, Hkv, hd, head_map):
        s = self.ref(src)
        if head_map == "div":
            self.ok(self.L.lt_op_attention_identity(self.P(s), ld, col0, self.P(self.new(dst, (B * N, H * hd))), B, N, H, Hkv, hd, 0, self.stream()),
                    "attention_identity")
            return
        # the mutated head map has no kernel: the V heads as they are (H = Hkv), then the wrong gather on the words
        tmp = self.new("_v_heads", (B * N, Hkv * hd))
        self.ok(self.L.lt_op_attention_identity(self.P(s), ld, col0, self.P(tmp), B, N, Hkv, Hkv, hd, 0, self.stream()), "attention_identity")
        idx = torch.tensor(head_index(H, Hkv, head_map), device="cuda")
        self.new(dst, (B * N, H * hd)).copy_(tmp.view(B * N, Hkv, hd)[:, idx].reshape(B * N, H * hd))

    def op_q_post(self, src, ld, col0, ln_w, ln_b, ln_eps, dst, B, N, heads, hd, table, out_scale, rope_mode, t, watershed, grid_w, cs_len):
        f = lambda r: self.P(self.ref(r))
        tt = None if t is None else self.ref(t)
        self.ok(self.L.lt_op_qk_norm_rope_ex(f(src), ld, col0, f(ln_w), f(ln_b), ln_eps, self.P(self.new(dst, (B, heads, N, hd))), B, N, heads, hd,
                                             rope_mode, f(table), cs_len, self.P(tt), watershed, grid_w, self.P(None), self.P(None), out_scale,
                                             self.P(None), self.P(None), 0, 0, self.stream()), "qk_norm_rope_ex")

    def op_attention_text(self, q, tk, tvt, tbias, tgate, dst, B, H, Hkv, N, T, Tpad, hd, tanh):
        f = lambda r: self.P(self.ref(r))
        scale = float(np.float32(1.0 / np.sqrt(np.float64(hd))))
        if tanh:     # accumulate mode onto the rows the identity step left (the buffer keeps its guards)
            self.ok(self.L.lt_op_attention(f(q), f(tk), f(tvt), f(tbias), self.P(self.b[dst]), f(tgate), 1, B, H, Hkv, N, T, Tpad, hd, scale, 1,
                                           self.stream()), "attention (text, accumulate)")
            return
        # the mutated gate has no kernel: the text attention alone, then the gate without tanh on the words
        tmp = self.new("_text", (B * N, H * hd))
        self.ok(self.L.lt_op_attention(f(q), f(tk), f(tvt), f(tbias), self.P(tmp), self.P(None), 0, B, H, Hkv, N, T, Tpad, hd, scale, 1, self.stream()),
                "attention (text)")
        g = self.ref(tgate).float().repeat_interleave(hd)
        self.b[dst].copy_((self.b[dst].float() + (tmp.float() * g).to(torch.bfloat16).float()).to(torch.bfloat16))


def pag_mutations(case, steps, P):
    """[(name, hook, gqa_only)] on the steps of `pag_steps`: each changes one argument of one step of a perturbed block"""
    cfg, fam = case.cfg, case.fam
    d, L, Hkv, hd = cfg.dim, cfg.n_layers, cfg.kv_heads, cfg.head_dim
    dkv = Hkv * hd
    by = {s.name: s.args for s in steps}
    out = []
    for l in sorted(P):
        p = f"layers.{l}.attention."
        if fam["text"]:
            out.append((f"l{l}.identity_reads_k_columns", FC.set_arg(f"l{l}.attn_id", col0=d), False))
        else:
            out.append((f"l{l}.identity_reads_k_columns", FC.set_arg(f"l{l}.v", w=("w", p + "wk.weight")), False))
        out.append((f"l{l}.head_map_modulo", FC.set_arg(f"l{l}.attn_id", head_map="mod"), True))
        if fam["text"]:
            other = (l + 1) % L
            a = by[f"l{l}.attn_text"]
            out.append((f"l{l}.text_step_dropped", FC.drop(f"l{l}.attn_text"), False))
            out.append((f"l{l}.text_gate_without_tanh", FC.set_arg(f"l{l}.attn_text", tanh=False), False))
            out.append((f"l{l}.text_keys_of_layer_{other}", FC.set_arg(f"l{l}.attn_text", tk=("buf", f"ky{other}"), tvt=("buf", f"vty{other}")), False))
            assert a["tk"] == ("buf", f"ky{l}") and a["tvt"] == ("buf", f"vty{l}")
    return out
