"""-m gpu: the engine's model evaluation equals its operator chain, word for word.

For every case the output of the public model class (models.NextDiT, models.imagenet.DiT_Llama, models.flag_dit.DiT_Llama; plain forward
and forward_with_cfg) is compared, as integers, with the `Ops` backend of tests/forward_chain.py: the same evaluation as a sequence of
lt_op_* calls on the test's own NaN-filled, guarded buffers with the test's own weight packing, wired from the oracle's statement of the
model (tests/test_forward_chain_cpu.py holds that statement to the oracle).  Then every mutation of forward_chain.mutations - one wiring
argument changed - must change at least one word of the chain's output, so that the equality says something about that argument.

Launches, at the fixtures' shapes (64 / 60 / 104 tokens, 128 / 120 / 208 rows, 384 rows in the batch of three):
  all families       mirrored: patchify, lt_op_gemm_bf16 with bias (patch embedder, final linear), eol fill, timestep features,
                     lt_op_linear_small_m (t-embedder, cap embedder, ONE adaLN launch over all layers + final), add, prep_mod, rope tables,
                     rmsnorm_mod, lt_op_gated_residual_norm (below the persistent GEMM's sizes no projection leaves row statistics, so
                     lt_op_proj_gated_residual_norm's streaming form does not run), the SwiGLU GEMM, lt_op_gemm_splitk_auto with the 256-slot
                     workspace for every plain projection (the launcher splits W2, K >= 1024), lt_op_unpatchify_cfg; the prompt preparation:
                     cast, mask_to_bias, cap_pool_ln, rmsnorm_mod, lt_op_gemm_bf16 (wk_y | wv_y), lt_op_qk_norm_rope without rotation,
                     lt_op_v_transpose; label_gather.  Nothing pinned.
  next_t2i, flag_t2i mirrored: lt_op_qkv_post (one launch below 2048 rows) and lt_op_attention_fused (text keys inside the launch; head_dim
                     72 one-wave kernel at 64 tokens, the ping-pong kernel at 60; head_dim 96 at 104 tokens).  Nothing pinned.
  imagenet           mirrored: lt_op_qkv_attention_small (head_dim 48, 64 tokens).  That entry fixes the q / k LayerNorm eps, so the
                     q / k eps mutation alone runs against a SECOND engine pinned with lt_engine_set_option("attn_small_fused", 0) and the
                     chain on projection + lt_op_qkv_post + lt_op_attention; the two engines differ by the ulps of the statistics'
                     summation order (tests/test_gpu_variants.py), so no equality is asserted between them.
  moe_time, moe_space, moe   (models.moe.DiT_Llama_TimeMoE / _SpaceMoE / DiT_Llama; 64 tokens, 128 rows, E = 8 / 8 / 4, 9 / 9 / 5 tiles of 256 sorted rows)
                     mirrored: the attention as for imagenet; lt_op_linear_small_m without bias over ALL layers' time routers stacked; lt_op_moe_route
                     (space router) or, family moe under moe_route_fused 1, the route_* arguments of lt_op_gated_residual_norm_ex; lt_op_moe_plan_ex
                     per layer and branch - free routing of the time branch runs moe_plan_time_kernel, the space branch moe_plan_kernel<4>, forced
                     routing of the time branch moe_plan_kernel<4>'s router; lt_op_gemm_grouped_gather with SwiGLU and lt_op_gemm_grouped at variant 0
                     (the 128 x 128 SwiGLU and the 64 x 128 small-M tiles: asserted by name); the closing steps through moe_ys / moe_pos / moe_wts.
                     lt_moe_routing_record must equal the chain's sel buffers exactly.  The engine's all-layers plan launch (moe_time_plan_hoist 1)
                     is compared against the chain's per-layer plans; the matrix moe_route_fused {0, 1} x moe_time_plan_hoist {0, 1} is set per engine.
                     One mutation - the fused router moved into the attention branch's closing step - cannot be launched at all: the operator
                     refuses routing outside its MoE kernel, and the test asserts that refusal by name.
                     Out of reach at these sizes: the grouped mode of the persistent kernel and the pair layout of the expert weights (both need
                     1.5 tiles of 256 x 256 per CU), the tail split, the plan kernel's larger register forms and generic walk (tests/test_moe_plan.py).
gemm_prefetch riders read only.  Gated by shape and not reached at these sizes: the fused QKV launch, the V^T epilogue, attn_q_fused, the pair
layout, the row-statistics (ystat) form of the closing steps - tests/test_gpu_forward_chain_large.py runs the same comparison where they are.
Graph replay: the default ("graph" 2) captures above 1024 rows only, so the call-order cases set "graph" 1 on their engine
(lt_engine_set_option, per engine) and check lt_graph_replays: the first call of the key is eager, the second captures and launches the
graph, the third replays it - staging copies, the RoPE table rebuilt in front of a replay after another key changed it.
cfg_channels = 4 has no keyword on the public classes: that case takes the model's engine (built, loaded and prepared by the class) and
calls lt_forward_cfg with an lt_step_args of its own (the C ABI's struct, include/lumina_dit.h)."""
import ctypes as C

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models

import exact_misc as M
import forward_chain as FC
from test_forward_chain_cpu import MUTATION_CASES, make_case

pytestmark = pytest.mark.gpu

_MODELS = {}
CLASS_FAMILIES = ("imagenet", "moe_time", "moe_space", "moe")


def _ctor(family):
    return {"next_t2i": models.NextDiT, "imagenet": models.imagenet.DiT_Llama, "flag_t2i": models.flag_dit.DiT_Llama,
            "moe_time": models.moe.DiT_Llama_TimeMoE, "moe_space": models.moe.DiT_Llama_SpaceMoE, "moe": models.moe.DiT_Llama}[family]


def _model(case):
    """the public model of the case's family holding the case's weights.  Guided calls share one model per weight set (engine and upload are
    reused); a plain forward reads the attention flags the last guided call left on the module, as the reference's does, so it gets a fresh one"""
    def make():
        m = _ctor(case.cfg.family)(**case.cfg.ctor_kwargs())
        m.load_state_dict(case.sd, strict=True)
        return m.eval().to("cuda", torch.bfloat16)
    if not case.use_cfg:
        return make()
    sig = (case.cfg.family, str(sorted(case.cfg.to_dict().items())), float(sum(float(v.double().sum()) for v in case.sd.values())))
    if sig not in _MODELS:
        _MODELS[sig] = make()
    return _MODELS[sig]


def engine_eval(case, model=None):
    model = model or _model(case)
    i = case.inputs
    x, t = i["x"].to("cuda", case.io_dtype), i["t"].cuda()
    fam = case.cfg.family
    if fam in CLASS_FAMILIES:
        y = i["labels"].cuda()
        return model.forward_with_cfg(x, t, y, case.cfg_scale) if case.use_cfg else model(x, t, y)
    cap, mask = i["cap"].to("cuda", torch.bfloat16), i["mask"].cuda()
    if not case.use_cfg:
        return model(x, t, cap, mask)
    kw = dict(base_seqlen=case.base_seqlen, proportional_attn=case.proportional_attn)
    if fam == "flag_t2i":
        return model.forward_with_cfg(x, t, cap, mask, case.cfg_scale, **kw)
    if case.cfg_channels == 3:
        return model.forward_with_cfg(x, t, cap, mask, case.cfg_scale, scale_factor=case.scale_factor, scale_watershed=case.scale_watershed, **kw)
    eng = model.engine(x, cap.shape[1])
    eng.prepare_prompt(cap, mask)
    a = _lib.LtStepArgs(cfg_scale=case.cfg_scale, scale_factor=case.scale_factor, scale_watershed=case.scale_watershed,
                        base_seqlen=int(case.base_seqlen or 0), proportional_attn=int(case.proportional_attn), latent_h=case.H, latent_w=case.W,
                        batch=case.B, io_dtype=_lib.LT_BF16 if case.io_dtype == torch.bfloat16 else _lib.LT_F32, cfg_channels=case.cfg_channels,
                        ntk_factor=1.0)
    out = torch.empty_like(x)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(eng.lib.lt_forward_cfg(eng.handle, C.c_void_p(x.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()), C.byref(a), s),
               "lt_forward_cfg")
    return out


def chain_eval(case, steps, hook=None):
    return FC.run(FC.Ops(case), steps, hook)


def assert_same_words(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    M.assert_bits(M.bits(got), M.bits(want), what)


EQUAL_CASES = [(name, mode) for fam, names in FC.GOLDENS.items() for name in names
               for mode in ("forward", "cfg4") + (("lin2", "ntk2") if fam == "next_t2i" else ())]


S128_SWIGLU, S64 = "gemm_bf16_pp<4,2,1,2,1,..,1,4> (128x128, SwiGLU)", "gemm_bf16_pp<2,4,1,1,0,..,1,4> (64x128)"


def moe_engine_and_chain(case, paths, model=None):
    """a mixture-of-experts case: the engine (options per engine, routing recorded) against the chain - every output word, every row's recorded
    selection against the chain's sel buffers, the grouped GEMMs' kernels by name.  -> (the engine's output, the chain's backend)"""
    model = model or _model(case)
    be = FC.Ops(case)
    want = FC.run(be, FC.build(case, paths))
    engine_eval(case, model)          # (the class builds its engine on the first call)
    eng = model._engine
    L, rows = case.cfg.n_layers, case.B * case.N
    opts = {"moe_route_fused": paths.get("route_fused"), "moe_time_plan_hoist": paths.get("time_plan_hoist")}
    try:
        for k, v in opts.items():
            if v is not None:
                eng.set_option(k, int(v))
        if case.forced is not None:
            eng.moe_routing_force(case.forced)
        eng.moe_routing_record(True)
        got = engine_eval(case, model)
        rec = eng.moe_routing_read(rows)
    finally:
        eng.moe_routing_record(False)
        eng.moe_routing_force(None)
        for k in opts:
            eng.set_option(k, None)
    assert_same_words(got, want, f"{case.name} {paths}")
    runs = {"time": 0, "space": 1}
    for l in range(L):
        for br, b in runs.items():
            if any(x == br for x, _ in case.fam["moe"]):
                mine = be.b[f"sel.l{l}.{br}"][:2 * rows].view(rows, 2).cpu().numpy()
                bad = (mine != rec[l, b]).any(1).nonzero()[0]
                assert bad.size == 0, (case.name, l, br, "rows whose recorded selection differs from the chain's", bad[:8].tolist(), mine[bad[:4]].tolist(),
                                       rec[l, b][bad[:4]].tolist())
            else:
                assert (rec[l, b] == -1).all()
    P_ = (2 * rows + case.cfg.num_experts * 255 + 255) // 256 * 256        # the sorted rows: moe_ffn's tile bound for the call's rows
    assert set(be.kernels) == {("w13", P_, 2 * case.cfg.ffn_hidden, case.cfg.dim), ("w2", P_, case.cfg.dim, case.cfg.ffn_hidden)}, be.kernels
    for key, kernel in be.kernels.items():
        assert kernel == (S128_SWIGLU if key[0] == "w13" else S64), (case.name, key, kernel)
    return got, be


@pytest.mark.parametrize("name,mode", EQUAL_CASES + [("nextdit_tiny", "batch6"), ("nextdit_tiny", "eps"), ("imagenet_tiny", "eps"), ("flag_tiny", "eps")] +
                         [(name, mode) for name in FC.MOE_GOLDENS for mode in ("cfg4-t2", "eps")])
def test_engine_equals_the_operator_chain(golden_dir, name, mode):
    """every golden (its own latent size: 64, 60 = 6 x 10 and 8 x 13 = 104 tokens; two layers; ragged caption masks of 16 / 8 and 13 / 5 valid
    keys in a 64-key tile), plain forward and guidance 4, both RoPE branches; the batch of three images; the small-row weights"""
    case, paths = make_case(golden_dir, name, mode)
    want = chain_eval(case, FC.build(case, paths))
    assert_same_words(engine_eval(case), want, case.name)
    if case.fam.get("moe"):       # ... and once more with the routing recorded
        moe_engine_and_chain(case, paths)


@pytest.mark.parametrize("hoist", [0, 1])
@pytest.mark.parametrize("route_fused", [0, 1])
@pytest.mark.parametrize("name", FC.MOE_GOLDENS)
def test_moe_option_matrix_equals_the_chain(golden_dir, name, route_fused, hoist):
    """moe_route_fused x moe_time_plan_hoist, set on the engine alone: the chain routes the space branch inside the closing step or in a launch of
    its own as the engine does, and plans the time branch layer by layer against the engine's one launch for all layers (hoist 1)"""
    case = FC.golden_case(golden_dir, name, "cfg4-t2")
    moe_engine_and_chain(case, {"route_fused": bool(route_fused), "time_plan_hoist": bool(hoist)})


@pytest.mark.parametrize("name", FC.MOE_GOLDENS)
def test_forced_routing_equals_the_chain(golden_dir, name):
    """lt_moe_routing_force with a table that replaces the free choice on every third row of every branch that runs (the experts shifted by one):
    the chain hands the same table to its router and plan steps.  The time branch then routes row by row on the single-workgroup plan kernel"""
    import numpy as np
    free = FC.golden_case(golden_dir, name, "cfg4-t2")
    got_free, be = moe_engine_and_chain(free, {})
    L, rows, E = free.cfg.n_layers, free.B * free.N, free.cfg.num_experts
    table = np.full((L, 2, rows, 2), -1, dtype=np.int32)
    for l in range(L):
        for br, b in (("time", 0), ("space", 1)):
            if any(x == br for x, _ in free.fam["moe"]):
                sel = be.b[f"sel.l{l}.{br}"][:2 * rows].view(rows, 2).cpu().numpy().copy()
                sel[::3] = np.sort((sel[::3] + 1) % E, axis=1)
                assert (sel[:, 0] != sel[:, 1]).all()
                table[l, b] = sel
    case = FC.golden_case(golden_dir, name, "cfg4-t2", forced=table)
    got, be2 = moe_engine_and_chain(case, {})
    assert not torch.equal(got, got_free)
    for l in range(L):        # (the record shows the table, both branches)
        for br, b in (("time", 0), ("space", 1)):
            if (table[l, b] >= 0).all():
                assert np.array_equal(be2.b[f"sel.l{l}.{br}"][:2 * rows].view(rows, 2).cpu().numpy(), table[l, b])


@pytest.mark.parametrize("over", [dict(io_dtype=torch.float32), dict(proportional_attn=False, base_seqlen=None), dict(cfg_channels=4)],
                         ids=["fp32_io", "no_proportional_attn", "cfg_channels_4"])
def test_engine_equals_the_operator_chain_call_variants(golden_dir, over):
    case = FC.golden_case(golden_dir, "nextdit_tiny", "cfg4", **over)
    want = chain_eval(case, FC.build(case))
    got = engine_eval(case)
    assert got.dtype == case.io_dtype
    assert_same_words(got, want, f"{case.name} {sorted(over)}")
    base = chain_eval(FC.golden_case(golden_dir, "nextdit_tiny", "cfg4"), FC.build(FC.golden_case(golden_dir, "nextdit_tiny", "cfg4")))
    if "io_dtype" in over:      # the same words, widened
        assert torch.equal(want.to(torch.bfloat16), base)
    else:                        # ... and the variant is a different evaluation
        assert not torch.equal(want, base)


def _fresh_model(case):
    m = _ctor(case.cfg.family)(**case.cfg.ctor_kwargs())
    m.load_state_dict(case.sd, strict=True)
    return m.eval().to("cuda", torch.bfloat16)


def _three_calls(case, model, eng, want):
    """the eager call, the capture call and the replay of one key: each equals the chain, and the replay counter says which was which"""
    r0 = eng.graph_replays()
    for call, replays in enumerate((0, 1, 2)):
        got = engine_eval(case, model)
        assert model._engine is eng
        assert eng.graph_replays() == r0 + replays, (case.name, "call", call + 1, eng.graph_replays() - r0)
        assert_same_words(got, want, f"{case.name} call {call + 1} ({('eager', 'capture + launch', 'replay')[call]})")


@pytest.mark.parametrize("name", ["nextdit_tiny_gqa", "imagenet_tiny", "flag_tiny"])
def test_eager_capture_and_replay_equal_the_chain(golden_dir, name):
    """a fresh model whose engine captures at every size ("graph" 1, set on that engine alone): the first, second and third call of a key"""
    case = FC.golden_case(golden_dir, name, "cfg4")
    model = _fresh_model(case)
    engine_eval(case, model)            # (the class builds, loads and prepares its engine; under the default option this call is eager)
    eng = model._engine
    assert eng.graph_replays() == 0
    eng.set_option("graph", 1)
    want = chain_eval(case, FC.build(case))
    try:
        _three_calls(case, model, eng, want)
        if case.cfg.family == "next_t2i":
            # a second key that rebuilds the shared RoPE table (scale factor 2, linear branch), then the first key's graph again: the table must be
            # rebuilt in front of the replay
            other = FC.golden_case(golden_dir, name, "lin2")
            _three_calls(other, model, eng, chain_eval(other, FC.build(other)))
            r = eng.graph_replays()
            assert_same_words(engine_eval(case, model), want, f"{case.name} replayed after {other.name}")
            assert eng.graph_replays() == r + 1
    finally:
        eng.set_option("graph", None)


@pytest.mark.parametrize("name,mode", MUTATION_CASES)
def test_every_mutation_changes_a_word_of_the_chain(golden_dir, name, mode):
    case, paths = make_case(golden_dir, name, mode)
    steps = FC.build(case, paths)
    model = _model(case)
    pinned = {}
    if case.cfg.family == "imagenet" and not paths.get("small_fused", True):
        pinned["attn_small_fused"] = 0
    if "route_fused" in paths:
        pinned["moe_route_fused"] = int(paths["route_fused"])
    eng = None
    if pinned:     # (per engine, never the process default; dropped again below)
        engine_eval(case, model)
        eng = model._engine
        for k, v in pinned.items():
            eng.set_option(k, v)
    try:
        got = engine_eval(case, model)
    finally:
        for k in pinned:
            eng.set_option(k, None)
    assert_same_words(got, chain_eval(case, steps), f"{case.name} unmutated")
    same = []
    for mname, hook in FC.mutations(case, steps):
        if mname.endswith(FC.REFUSED_BY_OPERATOR):      # routing on the way out exists in the MoE row kernel only: this wiring cannot be launched
            with pytest.raises(_lib.LuminaLibError, match="routing on the way out needs the MoE kernel"):
                chain_eval(case, steps, hook)
            continue
        mutated = chain_eval(case, steps, hook)
        if bool((M.bits(mutated) == M.bits(got)).all()):
            same.append(mname)
    assert not same, (case.name, "mutations that change no word of the output", same)
