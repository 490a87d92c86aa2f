"""-m gpu: the engine inside a graph the CALLER records (``torch.cuda.graph`` around ``forward`` / ``forward_with_cfg``).

The engine's own HIP-graph cache is guarded by tests/test_gpu_model.py; here the graph belongs to the caller, replays without the engine
hearing of it, and still has to meet the engine state that lives outside every graph: the weights' layout (row-major / pair), the shared
RoPE table, the prompt buffers.  Every comparison is ``torch.equal`` against the same evaluation made eagerly (option ``graph`` 0) on an
engine that never saw a capture: a replay and an eager call run the same kernels on the same words, so there is no tolerance to choose.

What cannot be recorded - everything that allocates, synchronises or copies from host memory - must be refused by name before it launches
anything, and leave the caller's capture valid."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import DiTEngine, EngineLimits
from oracle import synth

from gpu_util import rel_l2, set_option

pytestmark = pytest.mark.gpu

KW_A = dict(cfg_scale=4.0, base_seqlen=16, proportional_attn=True, scale_factor=1.0, scale_watershed=1.0)
KW_B = dict(cfg_scale=4.0, base_seqlen=16, proportional_attn=True, scale_factor=2.0, scale_watershed=0.3)  # the other RoPE key
KW_BIG = dict(cfg_scale=4.0, base_seqlen=4096, proportional_attn=True)


def _new_engine(cfg, sd_dev, graph=None):
    m = models.NextDiT(**cfg.ctor_kwargs())
    eng = DiTEngine(variant=_lib.LT_VARIANT_NEXT_T2I, dim=m.dim, n_layers=m.n_layers, n_heads=m.n_heads, n_kv_heads=m.n_kv_heads,
                    ffn_hidden=m.ffn_hidden, patch_size=m.patch_size, in_channels=m.in_channels, out_channels=m.out_channels,
                    cap_feat_dim=m.cap_feat_dim, qk_norm=m.qk_norm, norm_eps=m.norm_eps, limits=EngineLimits(), device=torch.device("cuda"))
    eng.load_state_dict(sd_dev)
    if graph is not None:
        eng.set_option("graph", graph)  # (this engine only)
    return eng


def _dev_state(cfg, seed):
    return {k: v.to("cuda", torch.bfloat16) for k, v in synth.synth_state_dict(cfg, seed=seed).items()}


def _capture(fn):
    """record ``fn()`` (engine calls on static tensors) on a side stream; returns the graph and what fn returned (static outputs)"""
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        out = fn()
    return g, out


def _replay(g, out):
    g.replay()
    return [o.clone() for o in out] if isinstance(out, (list, tuple)) else out.clone()


class _Diffs:
    """every step of a sequence is compared; the assertion at the end names all that differ, with their rel_l2"""

    def __init__(self):
        self.bad = []

    def check(self, label, got, ref):
        if torch.equal(got, ref):
            print(f"caller capture: {label}: equal")
            return
        fin = "finite" if bool(torch.isfinite(got.float()).all()) else "NOT finite"
        self.bad.append((label, "rel_l2 %.3e" % rel_l2(got, ref), fin))
        print(f"caller capture: {label}: DIFFERS, rel_l2 {rel_l2(got, ref):.3e}, {fin}")

    def done(self):
        assert not self.bad, self.bad


# ---- a. capture basics: the tiny fixture model (16 x 16 latent, 128 rows) -------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = _dev_state(cfg, int(g["seed_w"]))
    z = torch.from_numpy(g["z"]).to("cuda", torch.bfloat16)
    gen = torch.Generator().manual_seed(11)
    z2 = torch.randn(1, 4, 16, 16, generator=gen).repeat(2, 1, 1, 1).to("cuda", torch.bfloat16)
    t = torch.from_numpy(g["t"]).cuda().float()
    cap = torch.from_numpy(g["cap"]).to("cuda", torch.bfloat16)
    mask = torch.from_numpy(g["mask"]).to("cuda", torch.int32)
    ref = _new_engine(cfg, sd, graph=0)  # never sees a capture: the eager side of every comparison
    return dict(cfg=cfg, sd=sd, z=z, z2=z2, t=t, t_hi=torch.full((2,), 0.8, device="cuda"), cap=cap, cap2=(cap * 0.5).contiguous(), mask=mask, ref=ref)


def _eager(ref, x, t, cap, mask, use_cfg, kw):
    ref._prompt.clear()
    ref.prepare_prompt(cap, mask)
    return ref.forward(x, t, use_cfg=use_cfg, **kw).clone()


def test_capture_replays_new_inputs_new_prompt_and_the_other_rope_key(tiny):
    """forward_with_cfg and forward in ONE graph of the caller's.  Replays pick up new contents of the static x / t and a new prompt of the
    same shape prepared outside the graph; an eager evaluation of the other RoPE key in between rewrites the shared table, which the graph
    must rebuild for itself - and the eager key must find ITS table again after the graph's replay rewrote it.  The engine would replay its
    own cached graph for this key by now (option graph 1, fourth use): inside the caller's capture it must hand out plain launches, so
    graph_replays() does not move."""
    T = tiny
    ref = T["ref"]
    plain = dict(scale_factor=1.0, scale_watershed=0.0)
    d = _Diffs()
    try:
        set_option("graph", 1)
        eng = _new_engine(T["cfg"], T["sd"])
        eng.prepare_prompt(T["cap"], T["mask"])
        x_s, t_s = T["z"].clone(), T["t"].clone()
        for _ in range(3):  # warm-up: the first use of a key is eager by design, the second captures the engine's graph, the third replays it
            warm = eng.forward(x_s, t_s, use_cfg=True, **KW_A).clone()
            eng.forward(x_s, t_s, use_cfg=False, **plain)
        d.check("warm-up cfg", warm, _eager(ref, x_s, t_s, T["cap"], T["mask"], True, KW_A))
        assert eng.get_option("layout_pinned") == 0
        replays0 = eng.graph_replays()
        assert replays0 >= 2, replays0  # (the engine's own graph is live for both keys: it is what must NOT run inside the caller's)
        g, outs = _capture(lambda: [eng.forward(x_s, t_s, use_cfg=True, **KW_A), eng.forward(x_s, t_s, use_cfg=False, **plain)])
        assert eng.get_option("layout_pinned") == 1 and eng.graph_replays() == replays0

        def compare(label, cap):
            got = _replay(g, outs)
            d.check(label + " cfg", got[0], _eager(ref, x_s, t_s, cap, T["mask"], True, KW_A))
            d.check(label + " plain", got[1], _eager(ref, x_s, t_s, cap, T["mask"], False, plain))

        compare("first replay", T["cap"])
        x_s.copy_(T["z2"]); t_s.copy_(T["t"] * 0.5)
        compare("new x and t", T["cap"])
        eng._prompt.clear()
        eng.prepare_prompt(T["cap2"], T["mask"])  # outside the graph, same shapes: the graph reads it through fixed pointers
        compare("new prompt", T["cap2"])
        assert eng.graph_replays() == replays0  # three replays of the caller's graph: none of the engine's
        t_s.copy_(T["t_hi"])
        ref_b = _eager(ref, x_s, T["t_hi"], T["cap2"], T["mask"], True, KW_B)
        ref_a = _eager(ref, x_s, T["t_hi"], T["cap2"], T["mask"], True, KW_A)
        assert not torch.equal(ref_a, ref_b)  # the two keys really differ (NTK branch at t = 0.8)
        d.check("eager, other RoPE key", eng.forward(x_s, T["t_hi"], use_cfg=True, **KW_B).clone(), ref_b)
        compare("replay after the other RoPE key", T["cap2"])
        d.check("eager, other RoPE key, after the replay", eng.forward(x_s, T["t_hi"], use_cfg=True, **KW_B).clone(), ref_b)
        compare("replay again", T["cap2"])
        # graph 1 is still on: the eager evaluations above took the engine's cache (key B: first use, capture), the caller's graph took nothing
        rb = eng.graph_replays()
        _replay(g, outs)
        assert eng.graph_replays() == rb
    finally:
        set_option("graph", 2)
    d.done()


# ---- b. a change of regime after the capture: 2 layers at the 2B widths, 8192 rows (pair regime) against 512 rows (small-M kernels) ---------
def _wide_data():
    cfg = synth.NextDiTConfig(n_layers=2)
    sd_cpu = synth.synth_state_dict(cfg, seed=81)
    sd = {k: v.to("cuda", torch.bfloat16) for k, v in sd_cpu.items()}
    sd2 = {k: (v * 1.5 if k.endswith("attention.wo.weight") else v) for k, v in sd.items()}
    z, t, cap, mask = synth.synth_inputs(cfg, latent_hw=(128, 128), text_len=128, uncond_len=8, seed=82)
    zs, ts, _, _ = synth.synth_inputs(cfg, latent_hw=(32, 32), text_len=128, uncond_len=8, seed=83)
    W = dict(cfg=cfg, sd=sd, sd2=sd2, z=z.to("cuda", torch.bfloat16), t=t.cuda().float(), zs=zs.to("cuda", torch.bfloat16), ts=ts.cuda().float(),
             cap=cap.to("cuda", torch.bfloat16), mask=mask.to("cuda", torch.int32))
    ref = _new_engine(cfg, sd, graph=0)
    ref.prepare_prompt(W["cap"], W["mask"])
    W["ref_big"] = ref.forward(W["z"], W["t"], use_cfg=True, **KW_BIG).clone()
    W["ref_big_pair"] = ref.get_option("last_pair")
    W["ref_small"] = ref.forward(W["zs"], W["ts"], use_cfg=True, **KW_BIG).clone()
    W["ref_small_pair"] = ref.get_option("last_pair")
    ref.load_state_dict(sd2)
    ref.prepare_prompt(W["cap"], W["mask"])
    W["ref_big_w2"] = ref.forward(W["z"], W["t"], use_cfg=True, **KW_BIG).clone()
    W["ref"] = ref
    return W


@pytest.fixture(scope="module")
def wide():
    """the model, the inputs and the eager results of every sequence below, computed once and left unchanged"""
    return _wide_data()


class _Wide:
    def __init__(self, W):
        self.W, self.d = W, _Diffs()
        # without this the sequences below would pass vacuously on a machine where the threshold between the regimes moves
        assert W["ref_big_pair"] == 1 and W["ref_small_pair"] == 0, (W["ref_big_pair"], W["ref_small_pair"])
        self.eng = _new_engine(W["cfg"], W["sd"])
        self.eng.prepare_prompt(W["cap"], W["mask"])
        self.x_s, self.t_s = W["z"].clone(), W["t"].clone()
        self.g = self.out = None

    def big(self, label, ref="ref_big"):
        self.d.check(label, self.eng.forward(self.x_s, self.t_s, use_cfg=True, **KW_BIG).clone(), self.W[ref])
        return self.eng.get_option("last_pair")

    def small(self, label):
        self.d.check(label, self.eng.forward(self.W["zs"], self.W["ts"], use_cfg=True, **KW_BIG).clone(), self.W["ref_small"])
        return self.eng.get_option("last_pair")

    def capture(self):
        assert self.eng.get_option("layout_pinned") == 0
        self.g, self.out = _capture(lambda: self.eng.forward(self.x_s, self.t_s, use_cfg=True, **KW_BIG))
        assert self.eng.get_option("layout_pinned") == 1

    def replay(self, label, ref="ref_big"):
        self.d.check(label, _replay(self.g, self.out), self.W[ref])


def test_regime_i_small_and_big_eager_evaluations_after_the_capture(wide):
    """(i) eager big x 3 (the weights are in the pair layout), capture big, replay, eager small, replay, eager big, replay"""
    s = _Wide(wide)
    assert [s.big(f"eager big {i}") for i in range(3)] == [1, 1, 1]  # pair regime, the third through the engine's own graph
    s.capture()
    s.replay("replay")
    assert s.small("eager small") == 0
    s.replay("replay after eager small")
    assert s.big("eager big after the pin") == 0  # pinned: a big eager evaluation stays row-major
    s.replay("replay after eager big")
    s.d.done()


def test_regime_ii_capture_on_row_major_weights_then_an_eager_big_evaluation(wide):
    """(ii) eager small first, so the weights are row-major when big is captured; the next eager big evaluation must not convert them"""
    s = _Wide(wide)
    assert s.big("eager big") == 1
    assert s.small("eager small") == 0
    s.capture()
    assert s.big("eager big after the capture") == 0
    s.replay("replay after eager big")
    assert s.small("eager small after the capture") == 0
    s.replay("replay after eager small")
    s.d.done()


def test_regime_iii_new_weights_after_the_capture(wide):
    """(iii) capture big, upload every weight again (wo scaled by 1.5: lt_set_weight of every key converts to row-major first) and prepare the
    prompt again, replay: the result is the eager evaluation with the new weights"""
    s = _Wide(wide)
    assert s.big("eager big") == 1
    s.capture()
    s.eng.load_state_dict(wide["sd2"])
    s.eng.prepare_prompt(wide["cap"], wide["mask"])
    s.replay("replay with the new weights", "ref_big_w2")
    assert s.big("eager big with the new weights", "ref_big_w2") == 0
    s.replay("replay again", "ref_big_w2")
    assert not torch.equal(wide["ref_big_w2"], wide["ref_big"])
    s.d.done()


def test_regime_iv_pair_layout_switched_off_after_the_capture(wide):
    """(iv) capture big, option pair_layout 0, eager big, replay"""
    s = _Wide(wide)
    assert s.big("eager big") == 1
    s.capture()
    try:
        set_option("pair_layout", 0)
        assert s.big("eager big, pair_layout 0") == 0
        s.replay("replay after pair_layout 0")
    finally:
        set_option("pair_layout", 1)
    assert s.big("eager big, pair_layout 1 again") == 0
    s.replay("replay, pair_layout 1 again")
    s.d.done()


def test_refused_upload_converts_nothing(wide):
    """lt_set_weight validates the key and the element count BEFORE it converts the weights to row-major: after a refused upload a large
    evaluation finds them as it left them (layout_flips of the next sampler call = 0; a conversion there would be the refused upload's)"""
    eng = wide["ref"]  # never pinned
    eng.prepare_prompt(wide["cap"], wide["mask"])
    eng.forward(wide["z"], wide["t"], use_cfg=True, **KW_BIG)
    assert eng.get_option("last_pair") == 1 and eng.get_option("layout_pinned") == 0
    src = torch.zeros(7, 5, dtype=torch.bfloat16, device="cuda")
    shape = (C.c_int64 * 2)(7, 5)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = eng.lib.lt_set_weight(eng.handle, b"layers.0.attention.wo.weight", C.c_void_p(src.data_ptr()), _lib.LT_BF16, shape, 2, s)
    assert rc != 0 and b"35 elements given" in eng.lib.lt_last_error(), eng.lib.lt_last_error()
    rc = eng.lib.lt_set_weight(eng.handle, b"layers.0.attention.no_such.weight", C.c_void_p(src.data_ptr()), _lib.LT_BF16, shape, 2, s)
    assert rc != 0 and b"unknown weight key" in eng.lib.lt_last_error()
    out = eng.sample_ode(wide["z"], [0.0, 1.0], "euler", use_cfg=True, return_trajectory=False, **KW_BIG)
    assert eng.get_option("layout_flips") == 0 and eng.get_option("last_pair") == 1
    # (a refused upload also leaves the prompt prepared and the weights complete: the call above ran) one Euler step from the same slope
    assert torch.isfinite(out.float()).all()


# ---- c. refusals under capture --------------------------------------------------------------------------------------------------------------
def _refusal_cases(T, eng):
    """(entry point, call) - every call is made with device-resident, ready-typed operands: the Python plumbing around the C call then does
    nothing but allocate from the graph's pool"""
    z, t, cap, mask = T["z"], T["t"], T["cap"], T["mask"]
    lib, h = eng.lib, eng.handle
    grid = [0.0, 0.25, 0.5, 1.0]  # Euler, 3 stages
    xs = [z[0, :, :16, :16].contiguous(), z[1, :, :16, :8].contiguous()]
    perm = torch.arange(256, dtype=torch.int32, device="cuda").view(1, 256)
    ones = torch.ones(1, 4)
    src = torch.zeros(8, dtype=torch.bfloat16, device="cuda")
    noise = torch.zeros((1,) + tuple(z.shape), dtype=z.dtype, device="cuda")
    steps = torch.tensor([[0.1, 1.0, 1.0, 1.0, 1.0, 0.1, 0.3, 0.05]])
    coef = torch.ones(3, 2, 4)

    def set_weight():
        shape = (C.c_int64 * 1)(8)
        rc = lib.lt_set_weight(h, b"no.such.key", C.c_void_p(src.data_ptr()), _lib.LT_BF16, shape, 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "lt_set_weight")

    # the multi-view samplers through the C ABI itself (the Python wrappers ask for set_views first, which has not run: the engine holds no
    # tables, and the capture refusal comes before that check)
    z1, buf = z[:1].contiguous(), torch.empty_like(z[:1])
    garr = (C.c_float * len(grid))(*grid)
    carr = (C.c_float * coef.numel())(*coef.reshape(-1).tolist())
    av = eng._step_args(z1, 4.0, 1.0, 1.0, 16, True)
    av.batch = 2
    P = lambda x: C.c_void_p(x.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def sample_views():
        _lib.check(lib.lt_sample_views(h, P(z1), C.c_void_p(0), P(buf), garr, len(grid), _lib.LT_ODE_EULER, C.byref(av), stream()), "lt_sample_views")

    def sample_views_guided():
        _lib.check(lib.lt_sample_views_guided(h, P(z1), P(z1), P(z1), C.c_void_p(0), P(buf), garr, carr, len(grid), C.byref(av), stream()),
                   "lt_sample_views_guided")

    return [
        ("lt_forward_packed", lambda: eng.forward_packed(xs, t)),
        ("lt_forward_cfg_packed", lambda: eng.forward_cfg_packed([xs[0], xs[0]], t, **KW_A)),  # first packed call of this engine: its table is not allocated
        ("lt_sample_ode_adaptive", lambda: eng.sample_ode_adaptive(z, [0.0, 1.0], "dopri5", rtol=1e-2, atol=1e-2, use_cfg=True, **KW_A)),
        ("lt_prepare_prompt_regional", lambda: eng.prepare_prompt_regional(cap, mask, cap[:1].contiguous(), mask[:1].contiguous(), 1, 2)),
        ("lt_set_views", lambda: eng.set_views((perm, ones, ones), 16, 16)),
        ("lt_set_weight", set_weight),
        ("lt_sample_ode", lambda: eng.sample_ode(z, grid, "euler", use_cfg=True, **KW_A)),
        ("lt_sample_ode_packed", lambda: eng.sample_ode_packed([xs[0], xs[0]], grid, "euler", use_cfg=True, **KW_A)),
        ("lt_sample_ode_masked", lambda: eng.sample_ode_masked(z, grid, z, z, z, "euler", use_cfg=True, **KW_A)),
        ("lt_sample_ode_masked_packed", lambda: eng.sample_ode_masked_packed([xs[0], xs[0]], grid, [xs[0]] * 2, [xs[0]] * 2, [xs[0]] * 2, "euler",
                                                                             use_cfg=True, **KW_A)),
        ("lt_sample_ode_cfg_schedule", lambda: eng.sample_ode_cfg_schedule(z, grid, [4.0, 1.0, 4.0], "euler",
                                                                           **{k: v for k, v in KW_A.items() if k != "cfg_scale"})),
        ("lt_sample_sde", lambda: eng.sample_sde(z, noise, steps, None, "Euler", None, use_cfg=True, **KW_A)),
        ("lt_sample_views", sample_views),
        ("lt_sample_views_guided", sample_views_guided),
    ]


REFUSED = ["lt_forward_packed", "lt_forward_cfg_packed", "lt_sample_ode_adaptive", "lt_prepare_prompt_regional", "lt_set_views", "lt_set_weight",
           "lt_sample_ode", "lt_sample_ode_packed", "lt_sample_ode_masked", "lt_sample_ode_masked_packed", "lt_sample_ode_cfg_schedule",
           "lt_sample_sde", "lt_sample_views", "lt_sample_views_guided"]


@pytest.fixture(scope="module")
def refusing(tiny):
    """one engine for all refusals: had any refused call launched or latched something, the later cases and the closing test would see it"""
    eng = _new_engine(tiny["cfg"], tiny["sd"], graph=0)
    eng.prepare_prompt(tiny["cap"], tiny["mask"])
    before = eng.forward(tiny["z"], tiny["t"], use_cfg=True, **KW_A).clone()
    return dict(eng=eng, before=before)


@pytest.mark.parametrize("entry", REFUSED)
def test_entry_points_that_cannot_be_recorded_refuse_by_name_and_leave_the_capture_valid(tiny, refusing, entry):
    """the call returns a non-zero status whose message names the entry point and the capture; the caller's capture then ends normally and
    its other content - a plain tensor add - replays; nothing of the engine's was recorded or changed (no latch, same bits afterwards)"""
    eng = refusing["eng"]
    call = dict(_refusal_cases(tiny, eng))[entry]
    a = torch.arange(64, dtype=torch.float32, device="cuda")
    caught = []

    def body():
        try:
            call()
        except _lib.LuminaLibError as ex:
            caught.append(str(ex))
        return a + 1.0

    g, b = _capture(body)
    assert len(caught) == 1, f"{entry} was not refused on a capturing stream"
    assert entry in caught[0] and "capture" in caught[0], caught[0]
    a.mul_(2.0)
    g.replay()
    assert torch.equal(b, torch.arange(64, dtype=torch.float32, device="cuda") * 2.0 + 1.0)
    assert eng.get_option("layout_pinned") == 0 and eng.graph_replays() == 0
    assert torch.equal(eng.forward(tiny["z"], tiny["t"], use_cfg=True, **KW_A), refusing["before"])


def test_first_evaluation_of_a_model_is_refused_under_capture(tiny):
    """a model object whose engine does not exist yet (or whose weights changed) would create it and upload the weights inside the caller's
    capture - allocations and a synchronisation: refused by name, the capture stays valid; the same call made eagerly first is what works"""
    m = models.NextDiT(**tiny["cfg"].ctor_kwargs())
    m.load_state_dict({k: v.float().cpu() for k, v in tiny["sd"].items()}, strict=True)
    m = m.eval().to("cuda", torch.bfloat16)
    a = torch.ones(8, device="cuda")
    caught = []

    def body():
        try:
            m.forward_with_cfg(tiny["z"], tiny["t"], tiny["cap"], tiny["mask"], 4.0, base_seqlen=16, proportional_attn=True)
        except _lib.LuminaLibError as ex:
            caught.append(str(ex))
        return a * 3.0

    g, b = _capture(body)
    assert len(caught) == 1 and "lt_create" in caught[0] and "capture" in caught[0], caught
    a.fill_(2.0)
    g.replay()
    assert torch.equal(b, torch.full((8,), 6.0, device="cuda"))
    eager = m.forward_with_cfg(tiny["z"], tiny["t"], tiny["cap"], tiny["mask"], 4.0, base_seqlen=16, proportional_attn=True).clone()
    g2, out = _capture(lambda: m.forward_with_cfg(tiny["z"], tiny["t"], tiny["cap"], tiny["mask"], 4.0, base_seqlen=16, proportional_attn=True))
    assert torch.equal(_replay(g2, out), eager)
    assert torch.equal(eager, _eager(tiny["ref"], tiny["z"], tiny["t"], tiny["cap"], tiny["mask"], True, KW_A))


def test_a_shape_beyond_the_warm_engines_limits_is_refused_before_the_engine_is_dropped(tiny):
    """a warmed-up model holds an engine sized for its limits (256 text tokens here).  A call that needs a larger one would drop that engine -
    freeing every buffer a graph recorded earlier reads - and create another: on a capturing stream it is refused by name BEFORE the old
    engine is touched.  The capture ends and replays, the old engine is still the model's and evaluates the same bits, and the graph recorded
    before still replays them."""
    m = models.NextDiT(**tiny["cfg"].ctor_kwargs())
    m.load_state_dict({k: v.float().cpu() for k, v in tiny["sd"].items()}, strict=True)
    m = m.eval().to("cuda", torch.bfloat16)
    call = lambda cap, mask: m.forward_with_cfg(tiny["z"], tiny["t"], cap, mask, 4.0, base_seqlen=16, proportional_attn=True)
    eager = call(tiny["cap"], tiny["mask"]).clone()
    eng = m._engine
    g0, out0 = _capture(lambda: call(tiny["cap"], tiny["mask"]))
    T_big = eng.limits.max_text + 64
    cap_big = torch.zeros(2, T_big, tiny["cap"].shape[2], dtype=torch.bfloat16, device="cuda")
    cap_big[:, :tiny["cap"].shape[1]] = tiny["cap"]
    mask_big = torch.zeros(2, T_big, dtype=torch.int32, device="cuda")
    mask_big[:, :tiny["mask"].shape[1]] = tiny["mask"]
    a = torch.ones(8, device="cuda")
    caught = []

    def body():
        try:
            call(cap_big, mask_big)
        except _lib.LuminaLibError as ex:
            caught.append(str(ex))
        return a * 3.0

    g, b = _capture(body)
    assert len(caught) == 1 and "lt_create" in caught[0] and "capture" in caught[0], caught
    a.fill_(2.0)
    g.replay()
    assert torch.equal(b, torch.full((8,), 6.0, device="cuda"))
    assert m._engine is eng and eng.handle
    assert torch.equal(call(tiny["cap"], tiny["mask"]), eager)
    assert torch.equal(_replay(g0, out0), eager)
    # made eagerly, the larger call is what it always was: a new engine for the new limits (and the end of g0's buffers: DESIGN.md 7h)
    del g0, out0
    big = call(cap_big, mask_big)
    assert m._engine is not eng and m._engine.limits.max_text == T_big and torch.isfinite(big.float()).all()


def test_prompt_preparation_and_the_flat_packed_forward_are_recordable(tiny):
    """what DESIGN.md 7h lists as recordable beside forward / forward_with_cfg: lt_prepare_prompt inside the caller's graph (a replay prepares
    whatever the static caption tensor holds by then) and lt_forward_cfg_packed after the engine's first packed call (its size table travels
    as a kernel argument).  Replays against the eager engine, bit for bit, with new contents in every static tensor."""
    ref = tiny["ref"]
    eng = _new_engine(tiny["cfg"], tiny["sd"], graph=0)
    d = _Diffs()
    x_s, t_s, cap_s = tiny["z"].clone(), tiny["t"].clone(), tiny["cap"].clone()
    xs = [x_s[0, :, :16, :8], x_s[1, :, :16, :8]]  # (views of the static state: 2 x 32 tokens, halves of equal size)

    def prepare_and_run():
        eng._prompt.clear()
        eng.prepare_prompt(cap_s, tiny["mask"])
        return [eng.forward(x_s, t_s, use_cfg=True, **KW_A)] + list(eng.forward_cfg_packed(xs, t_s, **KW_A))

    warm = prepare_and_run()  # eager first: the first packed call allocates the table's device copy

    def ref_packed():
        ref._prompt.clear()
        ref.prepare_prompt(cap_s, tiny["mask"])
        return [o.clone() for o in ref.forward_cfg_packed(xs, t_s, **KW_A)]

    d.check("eager packed", warm[1].clone(), ref_packed()[0])
    g, outs = _capture(prepare_and_run)
    assert eng.get_option("layout_pinned") == 1
    for label in ("first replay", "new x, t and caption"):
        got, want = _replay(g, outs), ref_packed()
        d.check(label + ": cfg", got[0], _eager(ref, x_s, t_s, cap_s, tiny["mask"], True, KW_A))
        d.check(label + ": packed 0", got[1], want[0])
        d.check(label + ": packed 1", got[2], want[1])
        x_s.copy_(tiny["z2"]); t_s.mul_(0.5); cap_s.mul_(0.5)
    assert not torch.equal(got[0], warm[0])
    d.done()


def test_profiled_evaluation_is_refused_under_capture(tiny):
    """the event profile brackets launches with HIP events, which a graph cannot carry: an evaluation and a prompt preparation on a capturing
    stream are refused while it is on, and recorded once it is off"""
    eng = _new_engine(tiny["cfg"], tiny["sd"], graph=0)
    eng.prepare_prompt(tiny["cap"], tiny["mask"])
    eager = eng.forward(tiny["z"], tiny["t"], use_cfg=True, **KW_A).clone()
    eng.profile_enable(True)
    caught = []

    def body():
        for what in (lambda: eng.forward(tiny["z"], tiny["t"], use_cfg=True, **KW_A),
                     lambda: (eng._prompt.clear(), eng.prepare_prompt(tiny["cap"], tiny["mask"]))):
            try:
                what()
            except _lib.LuminaLibError as ex:
                caught.append(str(ex))
        return tiny["t"] + 1.0

    try:
        g, b = _capture(body)
    finally:
        eng.profile_enable(False)
    if os.environ.get("LT_NO_EVENT_PROFILE"):  # lt_profile_enable is a no-op then: nothing to refuse, both calls were recorded
        assert caught == [] and eng.get_option("layout_pinned") == 1
    else:
        assert len(caught) == 2 and all("capture" in c and "lt_profile_enable" in c for c in caught), caught
        assert "model evaluation" in caught[0] and "lt_prepare_prompt" in caught[1], caught
        assert eng.get_option("layout_pinned") == 0  # a refused evaluation pins nothing
    g.replay()
    assert torch.equal(b, tiny["t"] + 1.0)
    g2, out = _capture(lambda: eng.forward(tiny["z"], tiny["t"], use_cfg=True, **KW_A))
    assert torch.equal(_replay(g2, out), eager)
