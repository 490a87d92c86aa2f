"""GPU: a blurred-query evaluation equals its operator chain word for word (tests/seg_chain.py through the lt_op_* entries); every
chain mutation changes a word; the refusals of the C entries leave NaN outputs untouched; the ``sample.py`` driver and the transport front ends."""
import ctypes as C
import math

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import EngineLimits
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE

import exact_misc as M
import forward_chain as FC
import seg_chain as SC
from gpu_util import P, lib, stream
from test_gpu_slg import STEP_KW, _build, _counts, _deep
from test_pag_cpu import deep_case

pytestmark = pytest.mark.gpu

CTOR = {"next_t2i": lambda: models.NextDiT, "imagenet": lambda: models.imagenet.DiT_Llama, "flag_t2i": lambda: models.flag_dit.DiT_Llama}
SETS = [((1,), ()), ((0, 1), ()), ((3,), ()), ((0, 1, 2, 3), ()), ((1,), (2,))]
SIGMA = 0.8     # radius 3: reflected on the 8 x 8 and 4 x 8 grids of the small goldens
_CASES = {}


def _case(golden_dir, name, depth=4, small_fused=True):
    key = (name, depth, small_fused)
    if key not in _CASES:
        case = deep_case(golden_dir, name, depth)
        m = CTOR[case.cfg.family]()(**case.cfg.ctor_kwargs())
        m.load_state_dict(case.sd, strict=True)
        _CASES[key] = (case, FC.build(case, {"small_fused": small_fused}), FC.build(case, {"small_fused": False}), m.eval().to("cuda", torch.bfloat16))
    return _CASES[key]


def _sigma(case):
    return SIGMA if min(case.Hp, case.Wp) >= 4 else 0.3     # (radius 1 where a side of the grid is shorter than four tokens)


def _engine(case, model, Q=(), S=(), sigma=None):
    sigma = _sigma(case) if sigma is None else sigma
    i = case.inputs
    x, t = i["x"].to("cuda", case.io_dtype), i["t"].cuda()
    cond = (i["cap"].to("cuda", torch.bfloat16), i["mask"].cuda()) if case.fam["text"] else (i["labels"].cuda(),)
    return model.forward(x, t, *cond, blur_layers=list(reversed(Q)), skip_layers=list(S), blur_sigma=sigma)


def _same_words(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    M.assert_bits(M.bits(got), M.bits(want), what)


def _taps(sigma):
    mode, r, taps = G.seg_taps(sigma)
    return mode, taps.tolist()


def _engine_equals_chain(case, steps, plain_steps, model):
    base = _engine(case, model)
    _same_words(base, FC.run(SC.Ops(case), steps), f"{case.name} unblurred")
    mode, taps = _taps(_sigma(case))
    for Q, S in SETS:
        if max(Q + S) >= case.cfg.n_layers:
            continue
        want = FC.run(SC.Ops(case), SC.seg_steps(case, steps, plain_steps, Q, S, taps, mode))
        got = _engine(case, model, Q, S)
        _same_words(got, want, f"{case.name} Q={Q} S={S}")
        assert not torch.equal(got, base), (case.name, Q, S)
        assert torch.equal(_engine(case, model), base), (case.name, Q, S, "a set was left behind")
    # the mean query (sigma = inf) through the same chain
    want = FC.run(SC.Ops(case), SC.seg_steps(case, steps, plain_steps, (1,), (), [], 1))
    _same_words(_engine(case, model, (1,), (), math.inf), want, f"{case.name} mean query")


@pytest.mark.parametrize("name", ["nextdit_tiny", "nextdit_tiny_rect", "nextdit_tiny_gqa", "imagenet_tiny", "flag_tiny"])
def test_engine_equals_the_operator_chain(golden_dir, name):
    case, steps, plain, model = _case(golden_dir, name)
    _engine_equals_chain(case, steps, plain, model)


def test_engine_equals_the_chain_with_the_small_fused_route_off(golden_dir):
    case, steps, plain, model = _case(golden_dir, "imagenet_tiny", small_fused=False)
    _engine(case, model)     # (the class builds its engine on the first call)
    model._engine.set_option("attn_small_fused", 0)
    try:
        _engine_equals_chain(case, steps, plain, model)
    finally:
        model._engine.set_option("attn_small_fused", None)


def test_engine_equals_the_chain_at_head_dim_128(golden_dir):
    case, steps, plain, model = _case(golden_dir, "imagenet_tiny_hd128", depth=2, small_fused=False)
    assert case.cfg.head_dim == 128
    _engine_equals_chain(case, steps, plain, model)


@pytest.mark.parametrize("name", ["nextdit_tiny", "nextdit_tiny_gqa", "imagenet_tiny", "flag_tiny"])
def test_every_seg_mutation_changes_a_word(golden_dir, name):
    case, steps, plain, model = _case(golden_dir, name)
    Q = (1, 3)
    assert _sigma(case) == SIGMA
    mode, taps = _taps(SIGMA)
    qsteps = SC.seg_steps(case, steps, plain, Q, (), taps, mode)
    got = _engine(case, model, Q)
    _same_words(got, FC.run(SC.Ops(case), qsteps), f"{case.name} Q={Q}")
    other = _taps(0.5)[1]      # radius 2 in place of 3
    assert len(other) != len(taps)
    muts = SC.seg_mutations(case, qsteps, Q, other)
    assert len(muts) == len(Q) * (4 if case.fam["text"] else 3)
    for mname, hook in muts:
        assert not torch.equal(FC.run(SC.Ops(case), qsteps, hook), got), (case.name, mname)
    for l in Q:     # blur before RoPE: other steps, not a hook
        out = FC.run(SC.Ops(case), SC.seg_steps(case, steps, plain, Q, (), taps, mode, before_rope=l))
        assert not torch.equal(out, got), (case.name, l, "blur before RoPE")


# ---- refusals of the C entries: before any launch, NaN outputs untouched ------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    cfg, sd, (cap, cmask) = _deep(golden_dir, "next")
    model = _build("next", cfg, sd)
    n = 2 * 4 * 16 * 16
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    zs = z[:, :, :8, :8].contiguous()     # a 4 x 4 grid of tokens
    lim = model.engine_limits
    model.engine_limits = EngineLimits(max(lim.max_batch, 6), lim.max_tokens, lim.max_text)
    t = torch.full((2,), 0.5, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0).clone()
    eng, L = model._engine, lib()
    out = torch.full((8 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    grid = (C.c_float * 4)(0.0, 0.25, 0.5, 1.0)
    f3, i32 = C.c_float * 3, C.c_int32
    good, sgood, slate = f3(4.0, 1.0, 3.0), f3(2.0, 1.5, 0.0), f3(0.0, 0.0, 2.0)
    arr = lambda v: (i32 * max(len(v), 1))(*v)

    def call(*, x=z, tab=good, seg=sgood, skip=(2,), blur=(1,), sigma=1.0, method=0, batch=2, n_blur=None, null_blur=False):
        a = eng._step_args(x, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        return L.lt_sample_ode_cfg_seg(eng.handle, P(x), P(out), P(out[4 * n:]), grid, 4, method, tab, seg, arr(skip), len(skip),
                                       None if null_blur else arr(blur), len(blur) if n_blur is None else n_blur, sigma, 1, C.byref(a), stream())

    def fwd(*, x=z, w=4.0, s=2.0, skip=(2,), blur=(1,), sigma=1.0):
        a = eng._step_args(x, 4.0, 1.0, 1.0, None, False)
        return L.lt_forward_cfg_seg(eng.handle, P(x), P(t), P(out), w, s, arr(skip), len(skip), arr(blur), len(blur), sigma, C.byref(a), stream())

    def plain(*, x=z, skip=(), blur=(1,), sigma=1.0):
        a = eng._step_args(x, 4.0, 1.0, 1.0, None, False)
        return L.lt_forward_blur(eng.handle, P(x), P(t), P(out), C.byref(a), arr(skip), len(skip), arr(blur), len(blur), sigma, stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    who, who1, who2 = "lt_sample_ode_cfg_seg:", "lt_forward_cfg_seg:", "lt_forward_blur:"
    refused(call(batch=3), who, "even batch")
    refused(call(seg=None), who, "null argument")
    refused(call(method=_lib.LT_ODE_ABM2), who, "unknown method")
    refused(call(blur=(4,)), who, "blur index 4", "outside 0..3")
    refused(call(blur=(3, 1, 3)), who, "blur index 3 is repeated")
    refused(call(blur=(1, 2), skip=(2,)), who, "layer 2 is in the skip set and in the blur set")
    refused(call(skip=(0, 1, 2, 3), blur=()), who, "leaves no layer")
    refused(call(n_blur=-1), who, "negative")
    refused(call(null_blur=True, n_blur=2), who, "null argument", "blur_host")
    refused(call(skip=(), blur=()), who, "both layer sets are empty")
    for bad in (0.0, -1.0, float("nan")):
        refused(call(sigma=bad), who, "not positive")
        refused(fwd(sigma=bad), who1, "not positive")
        refused(plain(sigma=bad), who2, "not positive")
    # a radius the call's grid cannot reflect: sigma 2 is radius 6, the grid 4 x 4 - also when the first stages have scale 0
    refused(call(x=zs, sigma=2.0), who, "cannot be reflected")
    refused(call(x=zs, sigma=2.0, seg=slate), who, "cannot be reflected")
    refused(fwd(x=zs, sigma=2.0), who1, "cannot be reflected")
    refused(plain(x=zs, sigma=2.0), who2, "cannot be reflected")
    refused(fwd(blur=(7,)), who1, "outside 0..3")
    refused(fwd(blur=(2,)), who1, "skip set and in the blur set")
    refused(fwd(skip=(), blur=()), who1, "both layer sets are empty")
    refused(fwd(s=float("inf")), who1, "smoothed-energy scale is not finite")
    refused(plain(blur=(4,)), who2, "outside 0..3")
    refused(plain(blur=(1,), skip=(1,)), who2, "skip set and in the blur set")
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
    # the Python layers
    tg, tab, one = [0.0, 0.5, 1.0], [4.0, 4.0], [1.0, 1.0]
    sched = lambda **kw: model.sample_ode_cfg_schedule(z, tg, tab, cap, cmask, **{"method": "euler", "seg": one, "seg_layers": [1], "seg_sigma": 1.0, **kw})
    for kw, word in ((dict(rescale=0.5), "rescale / norm_limit"), (dict(reuse=[0, 1]), "guidance reuse"), (dict(method="ab2"), "fixed-grid"),
                     (dict(slg=one, slg_layers=[2]), "together with an slg table"), (dict(pag=one, pag_layers=[2]), "perturbed-attention"),
                     (dict(seg=[1.0]), "entries"), (dict(seg_sigma=None), "seg_sigma")):
        with pytest.raises(_lib.LuminaLibError, match=word):
            sched(**kw)
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.sample_ode_cfg_schedule([z[0], z[1]], tg, tab, cap, cmask, method="euler", seg=one, seg_layers=[1], seg_sigma=1.0)
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.forward([z[0], z[1]], t, cap, cmask, blur_layers=[1], blur_sigma=1.0)
    o = ODE(3, "euler", 4)
    ckw = dict(cap_feats=cap, cap_mask=cmask, cfg_scale=4.0)
    for kw, word in ((dict(teacache=0.1), "step caching"), (dict(pag_table=one, pag_layers=[2]), "perturbed-attention"), (dict(cfg_rescale=0.5), "rescale"),
                     (dict(cfg_apg=dict(eta=0.5)), "projected guidance"), (dict(seg_sigma=None), "seg_sigma")):
        with pytest.raises(ValueError, match=word):
            o.sample(z, model.forward_with_cfg, **{"cfg_table": tab, "seg_table": one, "seg_layers": [1], "seg_sigma": 1.0, **kw}, **ckw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # ... and the same arguments untouched are served; forward_with_cfg goes on as before
    assert call() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:4 * n].float()).all()) and eng.last_nfe() == 3 + 2 and eng.last_eval_rows() == (2 + 1) + (1 + 1) + 2
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0), ref)


# ---- the transport front ends and the driver ----------------------------------------------------------------------------------------------------
def test_class_conditional_family_through_the_transport_front_end(golden_dir):
    cfg, sd, (y,) = _deep(golden_dir, "imagenet")
    model = _build("imagenet", cfg, sd)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(9)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    o = ODE(5, "midpoint", 4)
    w = torch.tensor([1.0, 2.0, 2.0, 1.0, 4.0, 3.0, 3.0, 1.0])
    s = torch.tensor([0.0, 2.8, 0.0, 1.5, 0.0, -1.0, 2.0, 0.0])
    nfe, rows = _counts(w, s)
    kw = dict(y=y, cfg_scale=4.0)
    seg = dict(cfg_table=w, seg_table=s, seg_layers=[1, 3], seg_sigma=1.5, slg_layers=[2])
    got = o.sample(z, model.forward_with_cfg, **seg, **kw)
    assert model._engine.last_nfe() == nfe and model._engine.last_eval_rows() == rows
    o.use_engine = False
    want = o.sample(z, model.forward_with_cfg, **seg, **kw)
    for i in range(5):
        assert torch.equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    fn = Sampler(create_transport()).sample_ode(sampling_method="midpoint", num_steps=5, time_shifting_factor=4.0)
    via = fn(z, model.forward_with_cfg, **seg, **kw)
    assert torch.equal(via[-1], got[-1])


def test_sample_driver_with_seg_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    cfg, sd, _ = _deep(golden_dir, "next")
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_seg_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_seg_test"] = ctor
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
    on = ["--seg_layers", "1", "2", "--seg_scale", "3.0", "--seg_sigma", "1.5"]
    try:
        for name, extra in (("off", ["--seg_layers", "1", "2", "--seg_sigma", "1.5"]), ("seg", on)):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            runs[name] = (built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
        for extra, word in ((on + ["--cfg_rescale", "0.5"], "cfg_rescale"), (on + ["--slg_layers", "3", "--slg_scale", "1"], "slg_scale"),
                            (["--seg_scale", "2"], "need --seg_layers"), (on + ["--slg_layers", "1"], "disjoint"),
                            (on + ["--pag_layers", "3", "--pag_scale", "1"], "--pag_"), (["--seg_layers", "1", "--seg_scale", "2"], "needs --seg_sigma"),
                            (["--seg_layers", "1", "--seg_scale", "2", "--seg_sigma", "0"], "not positive"), (on + ["--teacache", "0.1"], "--teacache"),
                            (on + ["--cfg_reuse", "2"], "cfg_reuse")):
            with pytest.raises(SystemExit, match=word):
                S.run(S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / "no")]), encode_fn=encode,
                      cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
    finally:
        del models.__dict__["NextDiT_tiny_seg_test"]
    assert runs == {"off": (8, 16), "seg": (16, 24)}     # every evaluation of a run lies in ONE whole-trajectory call
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    feats, mask = encode(["a red cube", ""])
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    want = fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1]
    assert torch.equal(decoded[0], want / 0.13025)       # layers without a scale: the call it was
    fours = torch.full((8,), 4.0)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), feats, mask, 4.0, **kw)  # the flags the host loop's plain forward reads
    want = G.sample_cfg_seg(model, z, tgrid, fours, [3.0] * 8, [1, 2], 1.5, (), "midpoint", cap_feats=feats, cap_mask=mask, **kw)[-1][:1]
    assert torch.equal(decoded[1], want / 0.13025) and not torch.equal(decoded[1], decoded[0])
