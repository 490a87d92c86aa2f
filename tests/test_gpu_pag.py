"""GPU: perturbed-attention guidance - lt_op_attention_identity / lt_forward_perturb / lt_forward_cfg_pag / lt_sample_ode_cfg_pag.
Everything is exact: no tolerance.

* kernel: word for word against an index gather, NaN-filled guarded outputs, the pair layout brought back with lt_op_pair_layout, one shape
  beyond a pass of the capped grid, the refusals by name;
* engine = chain: ``model.forward(..., perturb_layers=P, skip_layers=S)`` equals the operator chain of tests/pag_chain.py run through the
  lt_op_* entries, on four-block models of every family, and every mutation of that chain changes a word; head_dim 128;
* pair plan: at the 2B width the perturbed forward under ``pair_layout`` 1 equals ``pair_layout`` 0;
* loop: the engine's trajectory equals ``transport.guidance.sample_cfg_pag`` state for state; graph keys; no set is left behind;
* refusals by name with the outputs untouched; the ``sample.py`` driver."""
import ctypes as C

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import EngineLimits
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

import exact_misc as M
import exact_rows as R
import forward_chain as FC
import pag_chain as PC
from gpu_util import P, lib, stream
from test_gpu_caller_capture import KW_BIG, _new_engine
from test_gpu_slg import DTYPES, STEP_KW, _build, _counts, _deep, _grid, _mixed
from test_pag_cpu import deep_case

pytestmark = pytest.mark.gpu

CAP_THREADS = 2048 * 256     # the launcher's capped grid: one pass of the stride loop


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- kernel ----------------------------------------------------------------------------------------------------------------------------------
def _kernel_case(B, N, H, Hkv, hd, pair, seed=0):
    L = lib()
    rows, col0 = B * N, 24
    ld = col0 + Hkv * hd + 16          # wider than the used columns, on both sides
    g = torch.Generator().manual_seed(100 * hd + 10 * N + B + seed)
    src = torch.randn(rows, ld, generator=g).mul(3).to("cuda", torch.bfloat16)
    kept = src.clone()
    buf = R.GuardedBuf(rows * H * hd, dtype=torch.bfloat16, fill=float("nan"))
    rc = L.lt_op_attention_identity(P(src), ld, col0, P(buf.out), B, N, H, Hkv, hd, pair, stream())
    assert rc == 0, L.lt_last_error()
    if pair:
        assert L.lt_op_pair_layout(P(buf.out), rows, H * hd, 0, stream()) == 0, L.lt_last_error()
    torch.cuda.synchronize()
    tag = (B, N, H, Hkv, hd, pair)
    buf.assert_intact(f"attention_identity {tag}")
    idx = torch.tensor([h // (H // Hkv) for h in range(H)], device="cuda")
    want = src[:, col0:col0 + Hkv * hd].reshape(rows, Hkv, hd)[:, idx].reshape(-1)
    got = buf.out.view(-1)
    assert torch.equal(_bits(got), _bits(want)), tag + (int((_bits(got) != _bits(want)).sum()),)
    assert torch.equal(_bits(src), _bits(kept)), tag


@pytest.mark.parametrize("pair", [0, 1], ids=["rowmajor", "pair"])
@pytest.mark.parametrize("H,Hkv,hd", [(4, 4, 48), (8, 2, 72), (2, 1, 96), (2, 2, 128)])
def test_kernel_word_for_word_against_an_index_gather(H, Hkv, hd, pair):
    ran = 0
    for B in (1, 3):
        for N in (1, 63, 64, 130):
            if pair and (B * N) % 2:
                continue     # (the pair layout holds row pairs: refused below)
            _kernel_case(B, N, H, Hkv, hd, pair)
            ran += 1
    assert ran == (4 if pair else 8)


@pytest.mark.parametrize("pair", [0, 1], ids=["rowmajor", "pair"])
def test_kernel_beyond_one_pass_of_the_capped_grid(pair):
    B, N, H, Hkv, hd = 1, 7400, 8, 2, 72
    assert B * N * (H * hd // 8) > CAP_THREADS
    _kernel_case(B, N, H, Hkv, hd, pair)


def test_kernel_refusals_by_name():
    L = lib()
    src = torch.zeros(64, 256, dtype=torch.bfloat16, device="cuda")
    out = torch.full((64 * 8 * 72 + 64,), float("nan"), dtype=torch.bfloat16, device="cuda")

    def call(s=src, o=out, ld=256, col0=8, B=1, N=64, H=4, Hkv=2, hd=48, pair=0):
        return L.lt_op_attention_identity(P(s), ld, col0, P(o), B, N, H, Hkv, hd, pair, stream())

    for kw, word in ((dict(s=None), "null argument"), (dict(o=None), "null argument"), (dict(H=5, Hkv=2), "not a multiple of Hkv"),
                     (dict(hd=64), "head_dim 64 not built"), (dict(hd=24), "head_dim 24 not built"), (dict(N=63, pair=1), "even row count"),
                     (dict(H=1, Hkv=1, hd=72, pair=1), "% 32 == 0"), (dict(col0=4), "col0 % 8 == 0"), (dict(ld=252), "ld_src % 8 == 0"),
                     (dict(col0=200), "inside a row"), (dict(o=out[1:]), "aligned"), (dict(B=0), "bad shape")):
        rc = call(**kw)
        msg = L.lt_last_error().decode()
        assert rc != 0 and "attention_identity" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0, L.lt_last_error()


# ---- engine = chain --------------------------------------------------------------------------------------------------------------------------
CTOR = {"next_t2i": lambda: models.NextDiT, "imagenet": lambda: models.imagenet.DiT_Llama, "flag_t2i": lambda: models.flag_dit.DiT_Llama,
        "moe": lambda: models.moe.DiT_Llama}
SETS = [((1,), ()), ((0, 1), ()), ((3,), ()), ((0, 1, 2, 3), ()), ((1,), (2,))]
_CASES = {}


def _case(golden_dir, name, depth=4, small_fused=True):
    """(case, paths, the chain's unperturbed steps, a fresh model of the public class with the case's weights), once per golden"""
    key = (name, depth, small_fused)
    if key not in _CASES:
        case = deep_case(golden_dir, name, depth)
        paths = {"small_fused": small_fused}
        m = CTOR[case.cfg.family]()(**case.cfg.ctor_kwargs())
        m.load_state_dict(case.sd, strict=True)
        _CASES[key] = (case, paths, FC.build(case, paths), m.eval().to("cuda", torch.bfloat16))
    return _CASES[key]


def _engine(case, model, P_=(), S=()):
    i = case.inputs
    x, t = i["x"].to("cuda", case.io_dtype), i["t"].cuda()
    cond = (i["cap"].to("cuda", torch.bfloat16), i["mask"].cuda()) if case.fam["text"] else (i["labels"].cuda(),)
    return model.forward(x, t, *cond, perturb_layers=list(reversed(P_)), skip_layers=list(S))


def _same_words(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    M.assert_bits(M.bits(got), M.bits(want), what)


def _engine_equals_chain(case, steps, model):
    plain = _engine(case, model)
    _same_words(plain, FC.run(PC.Ops(case), steps), f"{case.name} unperturbed")
    for P_, S in SETS:
        if max(P_ + S) >= case.cfg.n_layers:
            continue
        want = FC.run(PC.Ops(case), PC.pag_steps(case, steps, P_, S))
        got = _engine(case, model, P_, S)
        _same_words(got, want, f"{case.name} P={P_} S={S}")
        assert not torch.equal(got, plain), (case.name, P_, S)
        assert torch.equal(_engine(case, model), plain), (case.name, P_, S, "a set was left behind")
    return plain


@pytest.mark.parametrize("name", ["nextdit_tiny", "nextdit_tiny_rect", "nextdit_tiny_gqa", "imagenet_tiny", "flag_tiny", "moe_tiny"])
def test_engine_equals_the_operator_chain(golden_dir, name):
    case, _, steps, model = _case(golden_dir, name)
    _engine_equals_chain(case, steps, model)


def test_engine_equals_the_chain_with_the_small_fused_route_off(golden_dir):
    case, _, steps, model = _case(golden_dir, "imagenet_tiny", small_fused=False)
    _engine(case, model)     # (the class builds its engine on the first call)
    model._engine.set_option("attn_small_fused", 0)
    try:
        _engine_equals_chain(case, steps, model)
    finally:
        model._engine.set_option("attn_small_fused", None)


def test_engine_equals_the_chain_at_head_dim_128(golden_dir):
    case, _, steps, model = _case(golden_dir, "imagenet_tiny_hd128", depth=2, small_fused=False)
    assert case.cfg.head_dim == 128
    _engine_equals_chain(case, steps, model)


@pytest.mark.parametrize("name", ["nextdit_tiny", "nextdit_tiny_gqa", "imagenet_tiny", "flag_tiny"])
def test_every_pag_mutation_changes_a_word(golden_dir, name):
    case, _, steps, model = _case(golden_dir, name)
    P_ = (1, 3)
    psteps = PC.pag_steps(case, steps, P_)
    got = _engine(case, model, P_)
    _same_words(got, FC.run(PC.Ops(case), psteps), f"{case.name} P={P_}")
    gqa = case.cfg.kv_heads != case.cfg.n_heads
    seen = 0
    for mname, hook, gqa_only in PC.pag_mutations(case, psteps, P_):
        out = FC.run(PC.Ops(case), psteps, hook)
        if gqa_only and not gqa:
            assert torch.equal(out, got), (case.name, mname)     # H == Hkv: both head maps are the identity
        else:
            assert not torch.equal(out, got), (case.name, mname)
            seen += 1
    assert seen == len(P_) * ((4 if case.fam["text"] else 1) + int(gqa))


# ---- pair plan -------------------------------------------------------------------------------------------------------------------------------
def test_pair_plan_perturbed_forward_equals_the_row_major_plan():
    cfg = synth.NextDiTConfig(n_layers=2)
    sd = {k: v.to("cuda", torch.bfloat16) for k, v in synth.synth_state_dict(cfg, seed=81).items()}
    z, t, cap, mask = synth.synth_inputs(cfg, latent_hw=(128, 128), text_len=128, uncond_len=8, seed=82)
    z, t, cap, mask = z.to("cuda", torch.bfloat16), t.cuda().float(), cap.to("cuda", torch.bfloat16), mask.to("cuda", torch.int32)
    kw = dict(base_seqlen=KW_BIG["base_seqlen"], proportional_attn=True)
    eng = _new_engine(cfg, sd, graph=0)
    eng.prepare_prompt(cap, mask)
    res = {}
    for pair in (1, 0, 1):
        eng.set_option("pair_layout", pair)
        before = eng.forward(z, t, use_cfg=False, **kw).clone()
        assert eng.get_option("last_pair") == pair      # (the test says nothing on a machine where the threshold between the regimes moves)
        got = eng.forward(z, t, use_cfg=False, perturb_layers=[1], **kw).clone()
        assert eng.get_option("last_pair") == pair
        after = eng.forward(z, t, use_cfg=False, **kw)
        assert torch.equal(after, before), pair
        assert bool(torch.isfinite(got.float()).all()) and not torch.equal(got, before)
        for name, v in (("plain", before), ("perturbed", got)):
            if name in res:
                assert torch.equal(v, res[name]), (name, pair, int((v != res[name]).sum()))
            res[name] = v
    eng.set_option("pair_layout", None)


# ---- loop ------------------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _next_deep(golden_dir):
    if "next" not in _MODELS:
        cfg, sd, cond = _deep(golden_dir, "next")
        _MODELS["next"] = (_build("next", cfg, sd), cond)
    return _MODELS["next"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, (cap, cmask) = _next_deep(golden_dir)
    tgrid = _grid(method)
    w, s = _mixed(method)      # guided, conditional-only, s != 0 at w != 1 and s != 0 at w == 1
    assert len({(bool(a != 1), bool(b != 0)) for a, b in zip(w.tolist(), s.tolist())}) == 4
    nfe, rows1 = _counts(w, s)
    g = torch.Generator().manual_seed(6)
    z = torch.randn(1, 4, 16, 16, generator=g).to("cuda", dtype).repeat(2, 1, 1, 1)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), cap, cmask, 4.0, **STEP_KW)  # the flags a plain forward reads
    slg_only = model.sample_ode_cfg_schedule(z, tgrid, w, cap, cmask, method=method, return_trajectory=True, slg=s, slg_layers=[1], **STEP_KW)
    for pl, sl in (([2, 0], [1]), ([0, 1, 2, 3], [])):
        tag = (method, dtype, tuple(pl), tuple(sl))
        got = model.sample_ode_cfg_schedule(z, tgrid, w, cap, cmask, method=method, return_trajectory=True, pag=s, pag_layers=pl, slg_layers=sl,
                                            **STEP_KW)
        eng = model._engine
        assert eng.last_nfe() == nfe and eng.last_eval_rows() == rows1, tag + (eng.last_nfe(), eng.last_eval_rows())
        want = G.sample_cfg_pag(model, z, tgrid, w, s, pl, sl, method, cap_feats=cap, cap_mask=cmask, **STEP_KW)
        assert got.shape == want.shape == (len(tgrid),) + tuple(z.shape) and got.dtype == dtype and bool(torch.isfinite(want.float()).all()), tag
        for i in range(len(tgrid)):
            assert torch.equal(got[i], want[i]), tag + (i, int((got[i] != want[i]).sum()))
        assert not torch.equal(got[-1], slg_only[-1]), tag
    # P empty: skip-layer guidance; every s == 0: the schedule call
    assert torch.equal(model.sample_ode_cfg_schedule(z, tgrid, w, cap, cmask, method=method, return_trajectory=True, pag=s, pag_layers=[], slg_layers=[1],
                                                     **STEP_KW), slg_only)
    zeros = model.sample_ode_cfg_schedule(z, tgrid, w, cap, cmask, method=method, return_trajectory=True, pag=torch.zeros_like(s), pag_layers=[1], **STEP_KW)
    assert torch.equal(zeros, model.sample_ode_cfg_schedule(z, tgrid, w, cap, cmask, method=method, return_trajectory=True, **STEP_KW))


def test_class_conditional_family_through_the_transport_front_end(golden_dir):
    cfg, sd, (y,) = _deep(golden_dir, "imagenet")
    model = _build("imagenet", cfg, sd)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(9)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    o = ODE(5, "midpoint", 4)
    w = torch.tensor([1.0, 2.0, 2.0, 1.0, 4.0, 3.0, 3.0, 1.0])
    s = torch.tensor([0.0, 2.8, 0.0, 1.5, 0.0, -1.0, 2.0, 0.0])
    nfe, rows = _counts(w, s)
    kw = dict(y=y, cfg_scale=4.0)
    got = o.sample(z, model.forward_with_cfg, cfg_table=w, pag_table=s, pag_layers=[1, 3], slg_layers=[2], **kw)
    assert model._engine.last_nfe() == nfe and model._engine.last_eval_rows() == rows
    o.use_engine = False
    want = o.sample(z, model.forward_with_cfg, cfg_table=w, pag_table=s, pag_layers=[1, 3], slg_layers=[2], **kw)
    for i in range(5):
        assert torch.equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    fn = Sampler(create_transport()).sample_ode(sampling_method="midpoint", num_steps=5, time_shifting_factor=4.0)
    via = fn(z, model.forward_with_cfg, cfg_table=w, pag_table=s, pag_layers=[1, 3], slg_layers=[2], **kw)
    assert torch.equal(via[-1], got[-1])


def test_forward_with_cfg_pag_equals_the_host_expressions(golden_dir):
    model, (cap, cmask) = _next_deep(golden_dir)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(12)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    t = torch.full((2,), 0.25, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    assert torch.equal(model.forward_with_cfg_pag(z, t, cap, cmask, 4.0, pag_scale=0.0, pag_layers=[1], **STEP_KW), ref)
    got = model.forward_with_cfg_pag(z, t, cap, cmask, 4.0, pag_scale=2.8, pag_layers=[1, 3], skip_layers=[2], **STEP_KW)
    got1 = model.forward_with_cfg_pag(z, t, cap, cmask, 1.0, pag_scale=-1.5, pag_layers=[1, 3], **STEP_KW)
    o = model.forward(z, t, cap, cmask).to(torch.bfloat16)
    half = (z[:1], t[:1], cap[:1].contiguous(), cmask[:1].contiguous())
    k = model.forward(*half, skip_layers=[2], perturb_layers=[1, 3])
    k1 = model.forward(*half, perturb_layers=[1, 3])
    c, u = o[:1, :3], o[1:, :3]
    gch = G.slg_combine(c, u, k[:, :3], 4.0, 2.8)
    assert torch.equal(got, torch.cat([torch.cat([gch, gch]), o[:, 3:]], 1)) and not torch.equal(got, ref)
    r = torch.cat([G.slg_combine(c, None, k1[:, :3], 1.0, -1.5), o[:1, 3:]], 1)
    assert torch.equal(got1, torch.cat([r, r]))
    model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)


# ---- graphs and state --------------------------------------------------------------------------------------------------------------------------
def test_graph_path_five_keys_own_words_per_set_and_no_set_left_behind(golden_dir):
    cfg, sd, (cap, cmask) = _deep(golden_dir, "next")
    model = _build("next", cfg, sd)  # a fresh engine: no key has been used
    H, W = 50, 82  # 25 x 41 = 1025 tokens: the smallest latent whose B' = 1 evaluation has more than 1024 rows
    tgrid = ODE(7, "midpoint", 4).t  # 12 stages
    w1 = torch.tensor([2.0, 3.0, 1.0, 3.5, 1.0, 1.0, 5.0, 2.0, 1.0, 1.0, 4.0, 3.0])
    s1 = torch.tensor([2.8, 0.0, 0.0, 1.5, 2.0, 0.0, 0.0, -1.0, 3.0, 0.0, 0.0, 0.5])
    w2 = torch.tensor([1.0, 1.0, 4.5, 2.5, 2.0, 1.0, 1.0, 7.0, 3.0, 1.0, 1.0, 6.0])
    s2 = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.25, 2.0, 0.0, 4.0, 0.0, 1.0, 0.0, 3.0])
    z = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(8)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    t = torch.zeros(2, device="cuda")
    ref_cfg = model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    ref_plain = model.forward(z, t, cap, cmask)
    model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    eng = model._engine

    def kinds(w, s):  # how often each of the five keys is used: guided, cond-only, third, guided + s, cond + s
        g, on = w != 1, s != 0
        return [int((g & ~on).sum()), int((~g & ~on).sum()), int(on.sum()), int((g & on).sum()), int((~g & on).sum())]

    k1, k2 = kinds(w1, s1), kinds(w2, s2)
    assert all(c > 0 for c in k1) and all(c > 0 for c in k2) and k1 != k2
    run = lambda w, s, **kw: model.sample_ode_cfg_schedule(z, tgrid, w, cap, cmask, method="midpoint", return_trajectory=True, pag=s, **kw, **STEP_KW)
    before = eng.graph_replays()
    got = run(w1, s1, pag_layers=[1], slg_layers=[2])
    assert eng.graph_replays() - before == sum(k1) - 5     # the first use of a key runs eagerly, every later one replays
    mid = eng.graph_replays()
    other = run(w2, s2, pag_layers=[1], slg_layers=[2])
    assert eng.graph_replays() - mid == sum(k2)            # other table contents: the same five keys
    eng.set_option("graph", 0)
    try:
        eager, eager2 = run(w1, s1, pag_layers=[1], slg_layers=[2]), run(w2, s2, pag_layers=[1], slg_layers=[2])
    finally:
        eng.set_option("graph", None)
    assert torch.equal(got, eager) and torch.equal(other, eager2)
    # skip {1} and perturb {1} are two keys: three calls each in alternation give their own words
    want_skip = model.forward(z, t, cap, cmask, skip_layers=[1]).clone()
    want_pert = model.forward(z, t, cap, cmask, perturb_layers=[1]).clone()
    assert not torch.equal(want_skip, want_pert) and not torch.equal(want_pert, ref_plain)
    mid = eng.graph_replays()
    for rep in range(2):
        assert torch.equal(model.forward(z, t, cap, cmask, skip_layers=[1]), want_skip), rep
        assert torch.equal(model.forward(z, t, cap, cmask, perturb_layers=[1]), want_pert), rep
        assert torch.equal(model.forward(z, t, cap, cmask), ref_plain), rep
    assert eng.graph_replays() - mid >= 4     # (the second use of each key captured, the third replayed)
    eng.set_option("graph", 0)
    try:
        assert torch.equal(model.forward(z, t, cap, cmask, perturb_layers=[1]), want_pert)
    finally:
        eng.set_option("graph", None)
    # no set is left behind, also after refused calls
    for bad, word in ((dict(pag_layers=[1, 1]), "repeated"), (dict(pag_layers=[9]), "outside"), (dict(pag_layers=[1], slg_layers=[1]), "disjoint")):
        with pytest.raises(_lib.LuminaLibError, match=word):
            run(w1, s1, **bad)
        assert torch.equal(model.forward(z, t, cap, cmask), ref_plain), bad
    with pytest.raises(_lib.LuminaLibError):
        eng.forward(torch.zeros(2, 4, 15, 16, dtype=torch.bfloat16, device="cuda"), t, use_cfg=False, perturb_layers=[1])
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW), ref_cfg)
    assert torch.equal(model.forward(z, t, cap, cmask), ref_plain)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    cfg, sd, (cap, cmask) = _deep(golden_dir, "next")
    model = _build("next", cfg, sd)
    n = 2 * 4 * 16 * 16
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    lim = model.engine_limits
    model.engine_limits = EngineLimits(max(lim.max_batch, 6), lim.max_tokens, lim.max_text)
    t = torch.full((2,), 0.5, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0)
    eng, L = model._engine, lib()
    out = torch.full((8 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    grid = (C.c_float * 4)(0.0, 0.25, 0.5, 1.0)
    f3, i32 = C.c_float * 3, C.c_int32
    good, sgood, szero = f3(4.0, 1.0, 3.0), f3(2.0, 1.5, 0.0), f3(0.0, 0.0, 0.0)
    arr = lambda v: (i32 * max(len(v), 1))(*v)

    def call(*, tab=good, pag=sgood, skip=(2,), pert=(1,), method=0, batch=2, n_pert=None, null_pert=False):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        return L.lt_sample_ode_cfg_pag(eng.handle, P(z), P(out), P(out[4 * n:]), grid, 4, method, tab, pag, arr(skip), len(skip),
                                       None if null_pert else arr(pert), len(pert) if n_pert is None else n_pert, 1, C.byref(a), stream())

    def fwd(*, w=4.0, s=2.0, skip=(2,), pert=(1,)):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        return L.lt_forward_cfg_pag(eng.handle, P(z), P(t), P(out), w, s, arr(skip), len(skip), arr(pert), len(pert), C.byref(a), stream())

    def plain(*, skip=(), pert=(1,)):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        return L.lt_forward_perturb(eng.handle, P(z), P(t), P(out), C.byref(a), arr(skip), len(skip), arr(pert), len(pert), stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    who, who1, who2 = "lt_sample_ode_cfg_pag:", "lt_forward_cfg_pag:", "lt_forward_perturb:"
    refused(call(batch=3), who, "even batch")
    refused(call(pag=None), who, "null argument")
    refused(call(method=_lib.LT_ODE_ABM2), who, "unknown method")          # a multistep method
    refused(call(pert=(4,)), who, "perturb index 4", "outside 0..3")         # an index out of range
    refused(call(pert=(1, -1)), who, "perturb index -1", "outside 0..3")
    refused(call(pert=(3, 1, 3)), who, "perturb index 3 is repeated")        # a repeat
    refused(call(pert=(0, 1, 2, 3, 1), skip=()), who, "5 perturb indices", "4 layers")
    refused(call(pert=(1, 2), skip=(2,)), who, "layer 2 is in the skip set and in the perturb set")   # S and P meet
    refused(call(skip=(0, 1, 2, 3), pert=()), who, "leaves no layer")
    refused(call(n_pert=-1), who, "negative")
    refused(call(null_pert=True, n_pert=2), who, "null argument", "perturb_host")
    refused(call(skip=(), pert=()), who, "both layer sets are empty")
    refused(fwd(pert=(7,)), who1, "outside 0..3")
    refused(fwd(pert=(1, 1)), who1, "repeated")
    refused(fwd(pert=(2,)), who1, "skip set and in the perturb set")
    refused(fwd(skip=(), pert=()), who1, "both layer sets are empty")
    refused(fwd(s=float("inf")), who1, "perturbed-attention scale is not finite")
    refused(plain(pert=(4,)), who2, "outside 0..3")
    refused(plain(pert=(1,), skip=(1,)), who2, "skip set and in the perturb set")
    # a stream under capture: refused before anything is launched, the caller's capture stays valid
    a0 = torch.arange(64, dtype=torch.float32, device="cuda")
    graph, side, seen = torch.cuda.CUDAGraph(), torch.cuda.Stream(), []
    with torch.cuda.graph(graph, stream=side):
        for f in (call, fwd, plain):
            seen.append((f(), L.lt_last_error().decode()))
        b = a0 + 1.0
    for (rc, msg), name in zip(seen, (who, who1, who2)):
        assert rc != 0 and name in msg and "capture" in msg, (rc, msg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(b, a0 + 1.0) and bool(torch.isnan(out).all())
    # a regional prompt
    eng.prepare_prompt_regional(cap, cmask, cap[:1].contiguous(), cmask[:1].contiguous(), 1, 1)
    refused(call(), who, "regional prompt")
    refused(fwd(), who1, "regional prompt")
    refused(plain(), who2, "regional prompt")
    eng.prepare_prompt(cap, cmask)
    # the Python layer: a packed list, the rule, reuse, a multistep method, teacache, both tables
    tg, tab, one = [0.0, 0.5, 1.0], [4.0, 4.0], [1.0, 1.0]
    sched = lambda **kw: model.sample_ode_cfg_schedule(z, tg, tab, cap, cmask, **{"method": "euler", "pag": one, "pag_layers": [1], **kw})
    for kw, word in ((dict(rescale=0.5), "rescale / norm_limit"), (dict(reuse=[0, 1]), "guidance reuse"), (dict(method="ab2"), "fixed-grid"),
                     (dict(slg=one, slg_layers=[2]), "together with an slg table"), (dict(pag=[1.0]), "entries")):
        with pytest.raises(_lib.LuminaLibError, match=word):
            sched(**kw)
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.sample_ode_cfg_schedule([z[0], z[1]], tg, tab, cap, cmask, method="euler", pag=one, pag_layers=[1])
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.forward([z[0], z[1]], t, cap, cmask, perturb_layers=[1])
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.forward_with_cfg_pag([z[:1], z[:1]], t, cap, cmask, 4.0, pag_scale=1.0, pag_layers=[1])
    o = ODE(3, "euler", 4)
    with pytest.raises(ValueError, match="step caching"):
        o.sample(z, model.forward_with_cfg, cfg_table=tab, pag_table=one, pag_layers=[1], teacache=0.1, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # ... and the same arguments untouched are served; forward_with_cfg goes on as before
    assert call() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:4 * n].float()).all()) and eng.last_nfe() == 3 + 2 and eng.last_eval_rows() == (2 + 1) + (1 + 1) + 2
    assert call(pag=szero, skip=(), pert=()) == 0, L.lt_last_error()     # both sets empty at scale 0 everywhere: the schedule call
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0), ref)


# ---- driver ----------------------------------------------------------------------------------------------------------------------------------
def test_sample_driver_with_pag_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    cfg, sd, _ = _deep(golden_dir, "next")
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_pag_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_pag_test"] = ctor
    (tmp_path / "prompts.txt").write_text("a red cube\n")
    gen = torch.Generator().manual_seed(3)
    table = {c: torch.randn(16, cfg.cap_feat_dim, generator=gen) for c in ("a red cube", "")}

    def encode(caps):
        feats = torch.stack([table[c] for c in caps]).to("cuda", torch.bfloat16)
        mask = torch.ones(len(caps), 16, dtype=torch.int64, device="cuda")
        mask[-1, 8:] = 0
        return feats, mask

    decoded = []

    def decode(lat):
        decoded.append(lat.clone())
        return torch.sigmoid(lat[:, :3].float())

    argv = ["--ckpt", str(ck), "--caption_path", str(tmp_path / "prompts.txt"), "--resolution", "256:128x128", "--num_sampling_steps", "5",
            "--sampling-method", "midpoint", "--time_shifting_factor", "4", "--seed", "11"]
    fn = Sampler(create_transport()).sample_ode(sampling_method="midpoint", num_steps=5, time_shifting_factor=4.0)
    tgrid = fn.__self__.t
    runs = {}
    try:
        for name, extra in (("off", ["--pag_layers", "1", "2"]), ("pag", ["--pag_layers", "1", "2", "--pag_scale", "3.0"])):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            runs[name] = (built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
        for extra, word in ((["--pag_layers", "1", "--pag_scale", "2", "--cfg_rescale", "0.5"], "cfg_rescale"),
                            (["--pag_layers", "1", "--pag_scale", "2", "--slg_layers", "2", "--slg_scale", "1"], "slg_scale"),
                            (["--pag_scale", "2"], "need --pag_layers"), (["--pag_layers", "1", "--pag_scale", "2", "--slg_layers", "1"], "disjoint")):
            with pytest.raises(SystemExit, match=word):
                S.run(S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / "no")]), encode_fn=encode,
                      cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
    finally:
        del models.__dict__["NextDiT_tiny_pag_test"]
    assert runs == {"off": (8, 16), "pag": (16, 24)}     # every evaluation of a run lies in ONE whole-trajectory call
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    feats, mask = encode(["a red cube", ""])
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    want = fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1]
    assert torch.equal(decoded[0], want / 0.13025)       # layers without a scale: the call it was
    fours = torch.full((8,), 4.0)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), feats, mask, 4.0, **kw)  # the flags the host loop's plain forward reads
    want = G.sample_cfg_pag(model, z, tgrid, fours, [3.0] * 8, [1, 2], (), "midpoint", cap_feats=feats, cap_mask=mask, **kw)[-1][:1]
    assert torch.equal(decoded[1], want / 0.13025) and not torch.equal(decoded[1], decoded[0])
