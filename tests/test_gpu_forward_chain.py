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
gemm_prefetch riders read only.  Gated by shape and not reached at these sizes, so not covered here: the fused QKV launch, the V^T epilogue,
attn_q_fused, the pair layout, the row-statistics (ystat) form of the closing steps.
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


def _model(case):
    """the public model of the case's family holding the case's weights.  Guided calls share one model per weight set (engine and upload are
    reused); a plain forward reads the attention flags the last guided call left on the module, as the reference's does, so it gets a fresh one"""
    def make():
        ctor = {"next_t2i": models.NextDiT, "imagenet": models.imagenet.DiT_Llama, "flag_t2i": models.flag_dit.DiT_Llama}[case.cfg.family]
        m = ctor(**case.cfg.ctor_kwargs())
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
    if fam == "imagenet":
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


@pytest.mark.parametrize("name,mode", EQUAL_CASES + [("nextdit_tiny", "batch6"), ("nextdit_tiny", "eps"), ("imagenet_tiny", "eps"), ("flag_tiny", "eps")])
def test_engine_equals_the_operator_chain(golden_dir, name, mode):
    """every golden (its own latent size: 64, 60 = 6 x 10 and 8 x 13 = 104 tokens; two layers; ragged caption masks of 16 / 8 and 13 / 5 valid
    keys in a 64-key tile), plain forward and guidance 4, both RoPE branches; the batch of three images; the small-row weights"""
    case, paths = make_case(golden_dir, name, mode)
    want = chain_eval(case, FC.build(case, paths))
    assert_same_words(engine_eval(case), want, case.name)


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
    ctor = {"next_t2i": models.NextDiT, "imagenet": models.imagenet.DiT_Llama, "flag_t2i": models.flag_dit.DiT_Llama}[case.cfg.family]
    m = ctor(**case.cfg.ctor_kwargs())
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
    pinned = case.cfg.family == "imagenet" and not paths.get("small_fused", True)
    eng = None
    if pinned:     # (per engine, never the process default; dropped again below)
        engine_eval(case, model)
        eng = model._engine
        eng.set_option("attn_small_fused", 0)
    try:
        got = engine_eval(case, model)
    finally:
        if eng is not None:
            eng.set_option("attn_small_fused", None)
    assert_same_words(got, chain_eval(case, steps), f"{case.name} unmutated")
    same = []
    for mname, hook in FC.mutations(case, steps):
        mutated = chain_eval(case, steps, hook)
        if bool((M.bits(mutated) == M.bits(got)).all()):
            same.append(mname)
    assert not same, (case.name, "mutations that change no word of the output", same)
