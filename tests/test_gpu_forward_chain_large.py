"""-m gpu: the engine's model evaluation equals its operator chain, word for word, in the LARGE-ROW regime (tests/test_gpu_forward_chain.py is
the same comparison at the fixtures' 120-384 rows, where none of the routes below is taken).

From one 256-row tile per CU on, plan_block (csrc/engine.hip) sends a dense block down other launches; tests/forward_chain.py states them as
`paths` of its step list, this module runs the `Ops` backend of those lists - ROW-MAJOR throughout, on its own NaN-filled guarded buffers -
against the public model classes.  Two layers everywhere: the mid-block closing step reads the next layer's weights, the last one is the
final LayerNorm form (next_mode 2).  Weights: oracle.synth.synth_state_dict on configs made here; inputs from a seeded generator.

Cases (every one ASSERTS its regime before it compares and prints it: lt_op_gemm_qkv_fusable, the persistent kernel by name for O, W1 | W3 and
W2, the attention kernel by name, the row kernel of every closing step by name, "last_pair" after the engine's call):
  A   next_t2i, head_dim 72, GQA: d 2304 (H 32, Hkv 8, F 2304), 32 x 128 patches = 4096 tokens, 77 text keys with ragged masks, 4 rows = 16384.
      Mirrored: lt_op_qkv_qstat (fused QKV launch on 288-wide tiles with the Q partial sums, 16 slots, + the K pass), lt_op_attention_qraw_ex
      (q_norm + RoPE in the prologue, the kernel selects the table branch; text keys, bias and gate inside), lt_op_gemm_ystat for O and W2 and
      lt_op_gated_residual_norm_ex on their partial sums, the SwiGLU GEMM on the persistent kernel; the engine runs all of it in the pair layout.
      d is 2304 and not the 1152 of A': the streaming (ystat) row kernel exists for d = 1536 and 2304 only and for Next-DiT's mid-block form
      only (weighted post-norm, next pre-norm, no shift) - at every other width, and in EVERY last closing step (next_mode 2) and every
      Flag-DiT step, the projection still leaves the partial sums but the launcher takes the reducing kernel; the names printed say which.
  A'  next_t2i, head_dim 72: d 1152 (H 16, Hkv 4), 24 x 88 patches = 2112 tokens (a multiple of 64, not of 256: samples end inside a row
      tile), 8 rows = 16896 - max_batch is 8, and the V^T epilogue needs 64 row tiles at dkv 288, so 1344 tokens cannot reach it; scale_factor 2
      with t on either side of the watershed: both table branches through the prologue.
  B   flag_t2i, head_dim 96: d 1536 (H 16), 64 x (63 + eol) = 4096 tokens, 4 rows: 256-wide fused QKV tiles, lt_op_qk_norm_rope_pair (1-D RoPE:
      no prologue), the one-wave hd-96 kernel with the text keys inside, pair layout, ystat left and not read (shift chunks, no post-norm).
  C   imagenet, head_dim 48: d 1152 (H 24), 4096 tokens, 4 rows: the one-wave hd-48 kernel, pair layout, no text.
  D   imagenet, head_dim 128: d 1024 (H 8), 4096 tokens, 4 rows: fused QKV and ystat, NO pair layout (no one-wave kernel at 128: the
      attn_fwd_kernel_hd128 launch).  The engine refuses head_dim 128 with a text branch (lt_create), so this case is class-conditional; text
      keys in launches of their own are reached by the regional prompt path alone, which is out of scope below.
The printed regime is NOT the engine's own report: the library exposes the launchers' predicates (the describe entries, which see the process
default options) and, of the engine, "last_pair" alone.  That the engine took the fused launch, raw_q or the streaming row kernel is shown by
word equality with the chain that does, together with the assertion that the chains of two routes differ (below); for D, where last_pair is 0
by design, by nothing else.
Option matrix, per engine and restored: pair_layout {0, 1} (the chain is unchanged: the pair layout is promised bit-identical), grn_ystat
{1, 2} / {0} (the chain on ystat / on the reducing kernel), attn_q_fused 0 (the chain on lt_op_qk_norm_rope_pair), qkv_fused_gemm 0 (the chain on
lt_op_gemm_bf16 + lt_op_gemm_vt).  Every entry also compares its chain with the default route's: asserted different where the routes round
differently (A: ystat against the reducing kernel, the prologue against lt_op_qk_norm_rope_pair), printed otherwise - the V^T launch against the
fused one sums in the same order, and where no closing step streams (B - D) the ystat chain and the reducing chain are the same launches.  B - D
carry every setting too: pair_layout 1 and grn_ystat {1, 2} are the default or have no effect there, and must equal the default route.  Eager, capture and replay under the DEFAULT graph option; a regime flip on one engine (large, 64 tokens, large:
ensure_weight_layout converts the weights in place, both ways); one-argument mutations of the new steps (forward_chain.large_mutations) on A and C, two of them refusals asserted by name; the two refusals of
lt_op_gemm_ystat itself.
Still out of reach, deliberately: the regional prompt path, packed batches, the MoE families' grouped persistent mode and pair_moe; POST_SEPARATE
(qk_post_pair 0) has no path key.  The qstat SLOT COUNT is no argument of lt_op_qkv_qstat (it derives it), so no chain mutation stands in for
a wrong count in the engine: that one is covered by the engine-side trial recorded with the change (slots halved in block_attention: the
equality of A and A' fails)."""
import ctypes as C
import time

import pytest
import torch

import lumina_t2x_amd  # noqa: F401

import forward_chain as FC
from gpu_util import P, lib, ok, stream
from lumina_t2x_amd import _lib
from test_forward_chain_cpu import LARGE_PATHS
from test_gpu_forward_chain import _fresh_model, _three_calls, assert_same_words, engine_eval

pytestmark = pytest.mark.gpu

W4Q = "gemm_bf16_w4q<"
SPECS = {
    "A": dict(cfg=dict(dim=2304, n_heads=32, n_kv_heads=8, ffn_dim_multiplier=0.375), grid=(32, 128), rows=4, paths="qraw", pair=1,
              attn="attn_fwd_kernel_v4<72>", call=dict(scale_factor=2.0, scale_watershed=0.3), t=(0.6, 0.9)),
    "A'-lin": dict(cfg=dict(dim=1152, n_heads=16, n_kv_heads=4), grid=(24, 88), rows=8, paths="qraw", pair=1, attn="attn_fwd_kernel_v4<72>",
                   call=dict(scale_factor=2.0, scale_watershed=0.3), t=(0.1, 0.2, 0.25, 0.15)),
    "A'-ntk": dict(cfg=dict(dim=1152, n_heads=16, n_kv_heads=4), grid=(24, 88), rows=8, paths="qraw", pair=1, attn="attn_fwd_kernel_v4<72>",
                   call=dict(scale_factor=2.0, scale_watershed=0.3), t=(0.8, 0.5, 0.95, 0.35)),
    "B": dict(cfg=dict(dim=1536, n_heads=16, family="flag_t2i"), grid=(64, 63), rows=4, paths="pair", pair=1, attn="attn_fwd_kernel_v4h96", t=(0.4, 0.7)),
    "C": dict(cfg=dict(dim=1152, n_heads=24, family="imagenet", num_classes=10), grid=(64, 64), rows=4, paths="pair", pair=1,
              attn="attn_fwd_kernel_v4h48", t=(0.4, 0.7)),
    "D": dict(cfg=dict(dim=1024, n_heads=8, family="imagenet", num_classes=10), grid=(64, 64), rows=4, paths="pair", pair=0,
              attn="attn_fwd_kernel_hd128", t=(0.4, 0.7)),
}
T_TEXT = 77
_W, _CASES, _MODELS, _CHAINS, _CACHES = {}, {}, {}, {}, {}


def _weights(key):
    from oracle import synth
    sig = repr(sorted(SPECS[key]["cfg"].items()))
    if sig not in _W:
        cfg = synth.NextDiTConfig(n_layers=2, cap_feat_dim=256, **SPECS[key]["cfg"])
        _W[sig] = (cfg, synth.synth_state_dict(cfg, seed=11), sig)
    return _W[sig]


def case_of(key, grid=None, **over):
    """the guided call of a spec (rows = images cond + the same images uncond), or the same weights and prompt at another patch grid"""
    ck = (key, grid, repr(sorted((k, str(v)) for k, v in over.items())))
    if ck in _CASES:
        return _CASES[ck]
    sp = SPECS[key]
    cfg, sd, _ = _weights(key)
    hp, wp = grid or sp["grid"]
    n = sp["rows"] // 2
    gen = torch.Generator().manual_seed(23)
    z = torch.randn(n, cfg.in_channels, hp * cfg.patch_size, wp * cfg.patch_size, generator=gen)
    t = torch.tensor(sp["t"][:n])
    kw = dict(use_cfg=True, cfg_scale=4.0, name=f"large-{key}" + (f"-{hp}x{wp}" if grid else "") + "".join(f"-{k}" for k in sorted(over)), **sp.get("call", {}))
    if cfg.has_text:
        cap = torch.randn(2 * n, T_TEXT, cfg.cap_feat_dim, generator=gen)
        mask = torch.ones(2 * n, T_TEXT, dtype=torch.int32)
        for i in range(n):
            mask[i, T_TEXT - 9 * i - 3:] = 0      # ragged: 74, 65, ... valid keys, and 8 - i in the unconditional half
            mask[n + i, 8 - i:] = 0
        kw.update(cap=cap, mask=mask, base_seqlen=16, proportional_attn=True)
    else:
        kw.update(labels=torch.tensor([3, 7, 5, 1][:n] + [cfg.num_classes] * n))
    kw.update(over)
    x, t = (torch.cat([z, z]), torch.cat([t, t])) if kw["use_cfg"] else (torch.cat([z, z.flip(0)]), torch.cat([t, t]))
    _CASES[ck] = FC.Case(cfg, sd, x, t, **kw)
    return _CASES[ck]


def model_of(key):
    sig = _weights(key)[2]
    if sig not in _MODELS:
        _MODELS[sig] = _fresh_model(case_of(key))
    return _MODELS[sig]


def chain(case, paths_key, hook=None):
    """-> (the Ops backend's output of the case's list on `paths_key`, the row kernel of every closing step that was handed ystat); unmutated runs
    are cached per case and paths, weights and packed operands are shared per case (case names are unique here)"""
    ck = (case.name, paths_key)
    if hook is None and ck in _CHAINS:
        return _CHAINS[ck]
    be = FC.Ops(case)
    be.cache = _CACHES.setdefault(case.name, {})
    res = (FC.run(be, FC.build(case, LARGE_PATHS[paths_key] if paths_key else None), hook), dict(be.grn_kernels))
    if hook is None:
        _CHAINS[ck] = res
    return res


def _name(fn, *args):
    buf = C.create_string_buffer(200)
    ok(fn(*args, buf, 200), fn.__name__)
    return buf.value.decode()


def assert_regime(key, case, eng=None, pair=None):
    """the predicates the case means to run under, asserted and printed"""
    L, sp, cfg = lib(), SPECS[key], case.cfg
    d, dkv, hd, F, M, N = cfg.dim, cfg.kv_heads * cfg.head_dim, cfg.head_dim, cfg.ffn_hidden, case.B * case.N, case.N
    assert N % 64 == 0 and M % 2 == 0
    assert L.lt_op_gemm_qkv_fusable(M, d + 2 * dkv, d, d + dkv, N, hd) == 1, (key, "the QKV projection is not one launch", M, d + 2 * dkv)
    names = {"O": _name(L.lt_op_gemm_describe, M, d, d, 0, 0), "W1|W3": _name(L.lt_op_gemm_describe, M, 2 * F, d, 1, 0),
             "W2": _name(L.lt_op_gemm_describe, M, d, F, 0, 0)}
    for what, nm in names.items():
        assert nm.startswith(W4Q), (key, what, nm)
    fused_text = int(cfg.has_text)
    attn = _name(L.lt_op_attention_nk_describe, 0, 0, case.B, cfg.n_heads, cfg.kv_heads, N, N, N, hd, 0, fused_text, -(-case.T // 64) * 64 if fused_text else 0)
    assert attn == sp["attn"], (key, attn)
    _, grn = chain(case, sp["paths"])
    if eng is not None:
        assert eng.get_option("last_pair") == (sp["pair"] if pair is None else pair), (key, "last_pair", eng.get_option("last_pair"))
    print(f"{case.name}: M {M} = {case.B} x {N} tokens, d {d}, dkv {dkv}, F {F}; fused QKV launch; {names}; attention {attn}; closing steps {grn}; "
          f"last_pair {eng.get_option('last_pair') if eng is not None else '-'}")
    return grn


def engine_with(key, case, opts, model=None):
    """the engine's output under per-engine options, which are dropped again -> (output, last_pair)"""
    model = model or model_of(key)
    engine_eval(case, model)        # (the class builds its engine on the first call, and rebuilds it when the limits grow)
    eng = model._engine
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        got = engine_eval(case, model)
        assert model._engine is eng
        return got, eng.get_option("last_pair")
    finally:
        for k in opts:
            eng.set_option(k, None)


@pytest.mark.parametrize("key", list(SPECS))
def test_engine_equals_the_large_row_chain(key):
    t0 = time.time()
    case = case_of(key)
    want, _ = chain(case, SPECS[key]["paths"])
    model = model_of(key)
    got = engine_eval(case, model)
    grn = assert_regime(key, case, model._engine)
    assert_same_words(got, want, case.name)
    stream = [s for s, k in grn.items() if k.startswith("gated_residual_norm_ys_kernel")]
    if key == "A":      # the streaming row kernel runs in both mid-block steps of layer 0 and in layer 1's attention branch, and nowhere else
        assert sorted(stream) == ["l0.grn_attn", "l0.grn_ffn", "l1.grn_attn"], grn
    else:
        assert not stream, (key, grn)
    print(f"{case.name}: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("over", [dict(io_dtype=torch.float32), dict(use_cfg=False, scale_watershed=0.0, scale_factor=1.0, base_seqlen=None, proportional_attn=False)],
                         ids=["fp32_io", "plain_forward"])
def test_case_a_call_variants(over):
    case = case_of("A", **over)
    want, _ = chain(case, "qraw")
    model = _fresh_model(case) if not case.use_cfg else model_of("A")      # (a plain forward reads the flags the last guided call left on the module)
    got = engine_eval(case, model)
    assert got.dtype == case.io_dtype and model._engine.get_option("last_pair") == 1
    assert_same_words(got, want, f"{case.name} {sorted(over)}")
    base, _ = chain(case_of("A"), "qraw")
    if "io_dtype" in over:
        assert torch.equal(want.to(torch.bfloat16), base)
    else:
        assert not torch.equal(want, base)


MATRIX = [("A", {"pair_layout": 0}, "qraw", 0), ("A", {"pair_layout": 1}, "qraw", 1), ("A", {"grn_ystat": 1}, "qraw", 1), ("A", {"grn_ystat": 2}, "qraw", 1),
          ("A", {"grn_ystat": 0}, "qraw_reduce", 1), ("A", {"attn_q_fused": 0}, "pair", 1), ("A", {"qkv_fused_gemm": 0}, "qk_vt", 0),
          ("B", {"pair_layout": 0}, "pair", 0), ("B", {"grn_ystat": 0}, "pair_reduce", 1), ("B", {"qkv_fused_gemm": 0}, "qk_vt", 0),
          ("C", {"pair_layout": 0}, "pair", 0), ("C", {"grn_ystat": 0}, "pair_reduce", 1), ("C", {"qkv_fused_gemm": 0}, "qk_vt", 0),
          ("D", {"pair_layout": 0}, "pair", 0), ("D", {"grn_ystat": 0}, "pair_reduce", 0), ("D", {"qkv_fused_gemm": 0}, "qk_vt", 0)] + \
         [(k, o, "pair", SPECS[k]["pair"]) for k in "BCD" for o in ({"pair_layout": 1}, {"grn_ystat": 1}, {"grn_ystat": 2})]
MUST_DIFFER = {("A", "qraw_reduce"), ("A", "pair")}      # routes whose chains round differently: their words must not agree with the default's


@pytest.mark.parametrize("key,opts,paths_key,pair", MATRIX, ids=[f"{k}-{'-'.join(f'{n}{v}' for n, v in o.items())}" for k, o, _, _ in MATRIX])
def test_option_matrix_equals_the_chain(key, opts, paths_key, pair):
    case = case_of(key)
    want, _ = chain(case, paths_key)
    got, last_pair = engine_with(key, case, opts)
    print(f"{case.name} {opts}: chain on {paths_key} {LARGE_PATHS[paths_key]}, last_pair {last_pair}")
    assert last_pair == pair, (key, opts, last_pair)
    assert_same_words(got, want, f"{case.name} {opts}")
    base, _ = chain(case, SPECS[key]["paths"])
    if "pair_layout" in opts or opts.get("grn_ystat") in (1, 2):     # documented bit-identical to the default: the same words as the default engine's
        assert_same_words(got, base, f"{case.name} {opts} against the default route")
    elif paths_key != SPECS[key]["paths"]:
        differ = int((FC.M.bits(want) != FC.M.bits(base)).sum())
        print(f"{case.name}: chain on {paths_key} against the default route's: {differ} of {want.numel()} words differ")
        assert differ > 0 or (key, paths_key) not in MUST_DIFFER, (key, paths_key, "the two routes' chains agree: the entry cannot see the option")


@pytest.mark.parametrize("key", ["A", "A'-ntk", "B", "C", "D"])
def test_eager_capture_and_replay_under_the_default_graph_option(key):
    """a fresh engine, "graph" left at its default (2: captures above 1024 rows): the first, second and third call of one key"""
    case = case_of(key)
    want, _ = chain(case, SPECS[key]["paths"])
    model = _fresh_model(case)
    eng = model.engine(case.inputs["x"].to("cuda", case.io_dtype), case.T)      # (the class builds the engine; no evaluation has run on it)
    assert model._engine is eng
    assert eng.get_option("graph") == 2 and eng.graph_replays() == 0
    _three_calls(case, model, eng, want)
    assert eng.get_option("last_pair") == SPECS[key]["pair"]


def test_regime_flip_converts_the_weights_in_place_both_ways():
    """ONE engine: case A large (pair layout), the same weights at 64 tokens (row-major: the weights are converted back in place), large again"""
    big, small = case_of("A"), case_of("A", grid=(8, 8))
    model = _fresh_model(big)
    want_big, _ = chain(big, "qraw")
    want_small, _ = chain(small, None)
    engine_eval(big, model)
    eng = model._engine
    for n, (case, want, pair) in enumerate(((big, want_big, 1), (small, want_small, 0), (big, want_big, 1), (small, want_small, 0), (big, want_big, 1))):
        got = engine_eval(case, model)
        assert model._engine is eng
        assert eng.get_option("last_pair") == pair, (n, case.name, eng.get_option("last_pair"))
        assert eng.get_option("layout_flips") == 0      # (counts inside a sampler call only: lumina_dit_debug.h)
        assert_same_words(got, want, f"call {n + 1}: {case.name} after the other regime")


@pytest.mark.parametrize("key", ["A", "C"])
def test_every_large_mutation_changes_a_word_of_the_chain(key):
    case = case_of(key)
    pk = SPECS[key]["paths"]
    steps = FC.build(case, LARGE_PATHS[pk])
    got = engine_eval(case, model_of(key))
    want, grn = chain(case, pk)
    assert_same_words(got, want, f"{case.name} unmutated")
    muts = FC.large_mutations(case, steps)
    assert muts
    same, moved_unread = [], []
    for mname, hook in muts:
        if mname.startswith("gpu:refused:"):
            with pytest.raises(_lib.LuminaLibError, match=FC.LARGE_REFUSAL):
                chain(case, pk, hook)
            continue
        mutated, _ = chain(case, pk, hook)
        unchanged = bool((FC.M.bits(mutated) == FC.M.bits(got)).all())
        if mname.startswith("gpu:ystat:") and not grn[mname.split(":")[2]].startswith("gated_residual_norm_ys_kernel"):
            if not unchanged:       # this closing step's launcher has no streaming form: it must not read the partial sums at all
                moved_unread.append(mname)
        elif unchanged:
            same.append(mname)
    print(f"{case.name}: {len(muts)} mutations: {[m for m, _ in muts]}")
    assert not same, (case.name, "mutations that change no word of the output", same)
    assert not moved_unread, (case.name, "ystat changed a closing step whose kernel does not stream", moved_unread)


def test_gemm_ystat_refuses_by_name():
    """the debug entry's own refusals: a problem below one tile per CU (nothing would fill ystat), and a workspace narrower than the launch fills"""
    L = lib()
    a, w, c = (torch.zeros(256 * 2304, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    ws, n = torch.zeros(256 * 32, dtype=torch.float32, device="cuda"), C.c_int32(-1)
    assert L.lt_op_gemm_ystat(P(a), P(w), P(c), P(ws), 32, 256, 2304, 256, C.byref(n), stream()) != 0
    assert b"lt_op_gemm_ystat: this problem does not run on the persistent kernel's plain dense tiles (no ystat)" in L.lt_last_error(), L.lt_last_error()
    assert n.value == -1
    case = case_of("A")
    M, d = case.B * case.N, case.cfg.dim
    be = FC.Ops(case)
    be.cache = _CACHES.setdefault(case.name, {})
    wo = be.ref(("w", "layers.0.attention.wo.weight"))
    act, out = torch.zeros(M, d, dtype=torch.bfloat16, device="cuda"), torch.zeros(M, d, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(M, 2, dtype=torch.float32, device="cuda")
    assert L.lt_op_gemm_ystat(P(act), P(wo), P(out), P(ws), 2, M, d, d, C.byref(n), stream()) != 0
    assert b"lt_op_gemm_ystat: ystat workspace of 2 floats per row, the launch fills 16" in L.lt_last_error(), L.lt_last_error()
    assert n.value == -1 and not bool(out.any())       # (refused before anything was launched)
