"""GPU: skip-layer guidance - lt_forward_skip / lt_forward_cfg_slg / lt_sample_ode_cfg_slg / lt_op_unpatchify_cfg_slg.  Everything is
exact: no tolerance.

* kernel: store then guided, store then cond, against the torch bf16 chain word for word; guard words stay; one shape beyond a grid pass;
* layer skip: ``forward(skip_layers=S)`` equals (a) the plain forward of the same weights with the gate rows of the blocks in S zeroed - those
  blocks then add ``0 * y`` - and (b) the plain forward of a model rebuilt WITHOUT the blocks; four-block models of every family, one shape
  below and one above the 1024-row graph threshold;
* loop: the engine's trajectory equals the host loop ``transport.guidance.sample_cfg_slg`` state for state, with the counts the tables imply;
* graph path: at most five keys whatever the tables hold; no layer set is left behind, also after a refused call;
* identities, refusals by name with the outputs untouched, the other families through the transport front end, the ``sample.py`` driver."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import EngineLimits
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

import exact_slg as X
from gpu_util import P, lib, stream
from test_gpu_sde import _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
STEP_KW = dict(proportional_attn=True, base_seqlen=16)
GUARD = 64
_CACHE = {}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- kernel --------------------------------------------------------------------------------------------------------------------------
def _kernel_case(dtype, B, H, W, eol, scales=((4.0, 2.8), (1.5, -1.0), (0.0, 1.0), (-1.0, 0.0), (7.5, 0.375), (1.0, 3.0)), chs=(3, 4)):
    L = lib()
    Cc, out_ch, p = 4, 8, 2
    Hp, Wp = H // p, W // p
    stride = Wp + eol
    ws = stride if eol else 0
    ld = p * p * out_ch + 8
    half = B // 2
    g = torch.Generator().manual_seed(41 + B + 7 * eol + H)
    rows = torch.randn(B * Hp * stride, ld, generator=g).mul(3).to("cuda", torch.bfloat16)    # the stage's evaluation: 2 B' samples
    rows_k = torch.randn(half * Hp * stride, ld, generator=g).mul(3).to("cuda", torch.bfloat16)  # the skip evaluation: B' samples
    n = B * Cc * H * W
    code = _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32
    sentinel = 1.5

    def buf(count, dt=dtype):
        return torch.full((count + 2 * GUARD,), sentinel, dtype=dt, device="cuda")

    def guards_ok(t):
        return bool((t[:GUARD] == sentinel).all()) and bool((t[-GUARD:] == sentinel).all())

    def plain(src, b):  # the rows as a bf16 [b, C, H, W] tensor
        out = torch.empty(b * Cc * H * W, dtype=torch.bfloat16, device="cuda")
        assert L.lt_op_unpatchify_cfg(P(src), ld, P(out), _lib.LT_BF16, b, Cc, out_ch, H, W, p, 0, 1.0, 3, ws, stream()) == 0
        return out.view(b, Cc, H, W)

    o, ok = plain(rows, B), plain(rows_k, half)
    for ch in chs:
        nk = half * ch * H * W
        for w, s in scales:
            tag = (dtype, B, H, W, eol, ch, w, s)
            wd = torch.tensor([w], dtype=torch.float32, device="cuda")
            sd = torch.tensor([s], dtype=torch.float32, device="cuda")
            got, skip = buf(n), buf(nk, torch.bfloat16)
            untouched = got.clone()
            rc = L.lt_op_unpatchify_cfg_slg(P(rows_k), ld, P(got[GUARD:]), code, B, Cc, out_ch, H, W, p, None, None, ch, ws, P(skip[GUARD:]), 0, stream())
            assert rc == 0, L.lt_last_error()
            k = ok[:, :ch]
            assert torch.equal(_bits(skip[GUARD:-GUARD]), _bits(k.reshape(-1))), tag
            assert torch.equal(_bits(got), _bits(untouched)) and guards_ok(skip), tag  # store mode writes no out
            kept = skip.clone()
            # guided: all 2 B' rows
            rc = L.lt_op_unpatchify_cfg_slg(P(rows), ld, P(got[GUARD:]), code, B, Cc, out_ch, H, W, p, P(wd), P(sd), ch, ws, P(skip[GUARD:]), 1, stream())
            assert rc == 0, L.lt_last_error()
            c, u = o[:half, :ch], o[half:, :ch]
            gch = (u + w * (c - u)) + s * (c - k)
            exp = torch.cat([torch.cat([gch, o[:half, ch:]], 1), torch.cat([gch, o[half:, ch:]], 1)]).to(dtype).reshape(-1)
            assert torch.equal(_bits(got[GUARD:-GUARD]), _bits(exp)), tag + (int((got[GUARD:-GUARD] != exp).sum()),)
            assert guards_ok(got) and torch.equal(_bits(skip), _bits(kept)), tag
            # cond: the B' cond rows of another evaluation (here: the skip evaluation's own rows stand in for them)
            got = buf(n)
            rc = L.lt_op_unpatchify_cfg_slg(P(rows[: half * Hp * stride]), ld, P(got[GUARD:]), code, B, Cc, out_ch, H, W, p, None, P(sd), ch, ws,
                                            P(skip[GUARD:]), 2, stream())
            assert rc == 0, L.lt_last_error()
            r = torch.cat([c + s * (c - k), o[:half, ch:]], 1)
            exp = torch.cat([r, r]).to(dtype).reshape(-1)
            assert torch.equal(_bits(got[GUARD:-GUARD]), _bits(exp)), tag + (int((got[GUARD:-GUARD] != exp).sum()),)
            assert guards_ok(got) and torch.equal(_bits(skip), _bits(kept)), tag


@pytest.mark.parametrize("eol", [0, 1], ids=["grid", "eol"])
@pytest.mark.parametrize("H,W", [(4, 6), (6, 4)], ids=["4x6", "6x4"])
@pytest.mark.parametrize("B", [2, 6])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_kernel_store_guided_and_cond_word_for_word(dtype, B, H, W, eol):
    _kernel_case(dtype, B, H, W, eol)


def test_kernel_beyond_one_grid_pass():
    # the launcher caps its grid at 8192 blocks of 256 threads = 2 097 152 elements per pass; store and cond mode walk B' C H W = 2 130 048
    assert 2 * 4 * 516 * 516 > 8192 * 256
    _kernel_case(torch.bfloat16, 4, 516, 516, 1, scales=((4.0, 2.8),), chs=(3,))


def test_kernel_refusals():
    L = lib()
    rows = torch.zeros(2 * 6, 40, dtype=torch.bfloat16, device="cuda")
    out = torch.full((2 * 4 * 4 * 6,), float("nan"), dtype=torch.bfloat16, device="cuda")
    skip = torch.full((4 * 4 * 6,), float("nan"), dtype=torch.bfloat16, device="cuda")
    sc = torch.tensor([4.0], device="cuda")

    def call(B=2, ch=3, mode=1, k=skip, w=sc, s=sc, o=out):
        return L.lt_op_unpatchify_cfg_slg(P(rows), 40, P(o), _lib.LT_BF16, B, 4, 8, 4, 6, 2, P(w), P(s), ch, 0, P(k), mode, stream())

    for kw, word in ((dict(B=3), "even count"), (dict(ch=0), "cfg_channels"), (dict(ch=5), "cfg_channels"), (dict(mode=3), "mode 3"),
                     (dict(mode=-1), "mode -1"), (dict(k=None), "null argument"), (dict(s=None), "null argument"), (dict(w=None), "null argument"),
                     (dict(o=None), "null argument"), (dict(mode=2, s=None), "null argument")):
        rc = call(**kw)
        msg = L.lt_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg, word)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(skip).all())


# ---- layer skip, exact without a reference output ---------------------------------------------------------------------------------------
FAMILIES = {"next": ("nextdit_tiny", lambda: models.NextDiT), "imagenet": ("imagenet_tiny", lambda: models.imagenet.DiT_Llama),
            "flag": ("flag_tiny", lambda: models.flag_dit.DiT_Llama), "moe": ("moe_tiny", lambda: models.moe.DiT_Llama)}
DEPTH = 4
SETS = [(1,), (1, 2), (0, 1), (3,), (0, 2)]  # one block; an adjacent run; a run from layer 0 on; layer L - 1; layer 0 and a gap


def _deep(golden_dir, family, device="cuda"):
    """the family's small model of tests/golden with DEPTH blocks: (cfg, state dict, conditioning on ``device``)"""
    key = ("deep", family) if device == "cuda" else ("deep", family, device)
    if key not in _CACHE:
        name, _ = FAMILIES[family]
        g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
        cfg = dataclasses.replace(synth.NextDiTConfig(**json.loads(str(g["config"]))), n_layers=DEPTH)
        sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
        if cfg.has_text:
            cond = (torch.from_numpy(g["cap"]).to(device, torch.bfloat16), torch.from_numpy(g["mask"]).to(device))
        else:
            cond = (torch.from_numpy(g["y"]).to(device),)
        _CACHE[key] = (cfg, sd, cond)
    return _CACHE[key]


def _build(family, cfg, sd):
    m = FAMILIES[family][1]()(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=True)
    return m.eval().to("cuda", torch.bfloat16)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_forward_skip_equals_zeroed_gates_and_the_model_without_the_blocks(golden_dir, family):
    cfg, sd, cond = _deep(golden_dir, family)
    model = _build(family, cfg, sd)
    gen = torch.Generator().manual_seed(17)
    t = torch.tensor([0.25, 0.75], device="cuda")
    # 2 x 64 = 128 rows: plain launches; 2 x 24 x 24 = 1152 rows: above the 1024-row graph threshold
    shapes = [(16, 16), (48, 48)]
    zs = [torch.randn(2, 4, h, w, generator=gen).to("cuda", torch.bfloat16) for h, w in shapes]
    full = [model.forward(z, t, *cond) for z in zs]
    assert all(bool(torch.isfinite(f.float()).all()) for f in full)
    for S in SETS:
        identity = _build(family, cfg, X.zero_gates(sd, cfg.family, S, cfg.dim))
        cut_cfg = dataclasses.replace(cfg, n_layers=DEPTH - len(S))
        cut = _build(family, cut_cfg, X.drop_layers(sd, S))
        for z, f in zip(zs, full):
            tag = (family, S, tuple(z.shape))
            want = identity.forward(z, t, *cond)
            assert torch.equal(cut.forward(z, t, *cond), want), tag  # the two oracles agree
            assert not torch.equal(want, f), tag
            before = model._engine.graph_replays() if model._engine is not None else 0
            for rep in range(3):  # above the threshold: an eager run, the capture and its replay, a replay
                got = model.forward(z, t, *cond, skip_layers=list(reversed(S)))  # (any order)
                assert torch.equal(got, want), tag + (rep, int((got != want).sum()))
            assert model._engine.graph_replays() - before == (2 if z.shape[-1] == 48 else 0), tag
            # no set is left behind
            assert torch.equal(model.forward(z, t, *cond), f), tag
        del identity, cut
    # an empty set is the plain forward
    assert torch.equal(model.forward(zs[0], t, *cond, skip_layers=[]), full[0])


def test_forward_skip_refusals_leave_no_set_behind(golden_dir):
    cfg, sd, cond = _deep(golden_dir, "next")
    model = _build("next", cfg, sd)
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4)).to("cuda", torch.bfloat16)
    t = torch.tensor([0.25, 0.75], device="cuda")
    ref = model.forward(z, t, *cond)
    for bad, words in (([4], ("lt_forward_skip:", "outside 0..3")), ([-1], ("lt_forward_skip:", "outside 0..3")),
                       ([1, 2, 1], ("lt_forward_skip:", "repeated")), ([0, 1, 2, 3], ("lt_forward_skip:", "leaves no layer")),
                       ([0, 1, 2, 3, 0], ("lt_forward_skip:", "5 skip indices"))):
        with pytest.raises(_lib.LuminaLibError) as exc:
            model.forward(z, t, *cond, skip_layers=bad)
        assert all(w in str(exc.value) for w in words), str(exc.value)
        assert torch.equal(model.forward(z, t, *cond), ref), bad
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.forward([z[0], z[1]], t, *cond, skip_layers=[1])
    with pytest.raises(_lib.LuminaLibError, match="not an integer"):
        model.forward(z, t, *cond, skip_layers=[1.5])
    # a set, then a failing evaluation behind it (a latent the patch size does not divide), then the plain forward
    eng = model._engine
    with pytest.raises(_lib.LuminaLibError):
        eng.forward(torch.zeros(2, 4, 15, 16, dtype=torch.bfloat16, device="cuda"), t, use_cfg=False, skip_layers=[1])
    assert torch.equal(model.forward(z, t, *cond), ref)


# ---- loop ----------------------------------------------------------------------------------------------------------------------------
def _next_deep(golden_dir):
    if "next_model" not in _CACHE:
        cfg, sd, cond = _deep(golden_dir, "next")
        _CACHE["next_model"] = (_build("next", cfg, sd), cond)
    return _CACHE["next_model"]


def _grid(method):
    return ODE(5, method, 4).t  # a 5-point shifted grid: 4 / 8 / 16 evaluations


def _mixed(method):
    """(w, s): guided, conditional-only, s != 0 at w != 1 and s != 0 at w == 1 stages"""
    n = 4 * STAGES[method]
    w = [4.0, 1.0, 3.0, 1.0, 2.5, 1.0, 4.0, 1.0, 5.0, 1.5, 1.0, 1.0, 3.5, 3.0, 1.0, 4.0][:n]
    s = [2.8, 0.0, 0.0, 1.5, -1.0, 0.0, 0.0, 2.0, 0.375, 0.0, 3.0, 0.0, 0.0, 2.8, 2.8, 0.0][:n]
    return torch.tensor(w), torch.tensor(s)


def _counts(w, s):
    """(evaluations, rows per B' = 1) the tables imply: a skip evaluation is one more evaluation of B' rows"""
    guided, on = w != 1, s != 0
    nfe = len(w) + int(on.sum())
    rows = 2 * int(guided.sum()) + int((~guided).sum()) + int(on.sum())
    return nfe, rows


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, (cap, cmask) = _next_deep(golden_dir)
    tgrid = _grid(method)
    w, s = _mixed(method)
    kinds = {(bool(a != 1), bool(b != 0)) for a, b in zip(w.tolist(), s.tolist())}
    assert len(kinds) == 4  # all four kinds of stage
    nfe, rows1 = _counts(w, s)
    layers = [2, 1]
    g = torch.Generator().manual_seed(6)
    for B, H, W in ((2, 16, 16), (4, 16, 24)):
        Bh = B // 2
        tag = (method, dtype, B)
        z = torch.randn(Bh, 4, H, W, generator=g).to("cuda", dtype).repeat(2, 1, 1, 1)
        cf, cm = (cap, cmask) if B == 2 else (torch.cat([cap, cap.flip(0)]), torch.cat([cmask, cmask.flip(0)]))
        model.forward_with_cfg(z, torch.zeros(B, device="cuda"), cf, cm, 4.0, **STEP_KW)  # the flags a plain forward reads
        got = model.sample_ode_cfg_schedule(z, tgrid, w, cf, cm, method=method, return_trajectory=True, slg=s, slg_layers=layers, **STEP_KW)
        eng = model._engine
        assert eng.last_nfe() == nfe and eng.last_eval_rows() == Bh * rows1, tag + (eng.last_nfe(), eng.last_eval_rows())
        want = G.sample_cfg_slg(model, z, tgrid, w, s, layers, method, cap_feats=cf, cap_mask=cm, **STEP_KW)
        assert got.shape == want.shape == (len(tgrid),) + tuple(z.shape) and got.dtype == dtype, tag
        assert bool(torch.isfinite(want.float()).all()), tag
        for i in range(len(tgrid)):
            assert torch.equal(got[i], want[i]), tag + (i, int((got[i] != want[i]).sum()))
        final = model.sample_ode_cfg_schedule(z, tgrid, w, cf, cm, method=method, slg=s, slg_layers=layers, **STEP_KW)
        assert torch.equal(final, got[-1]), tag
        # the slg stages are not what plain guidance computes ...
        full = model.sample_ode_cfg_schedule(z, tgrid, w, cf, cm, method=method, return_trajectory=True, **STEP_KW)
        assert not torch.equal(full[-1], got[-1]), tag
        # ... and an all-zero slg table is the schedule call, bit for bit, half-row stages included
        zeros = model.sample_ode_cfg_schedule(z, tgrid, w, cf, cm, method=method, return_trajectory=True, slg=torch.zeros_like(s), slg_layers=layers,
                                              **STEP_KW)
        assert eng.last_nfe() == len(w) and eng.last_eval_rows() == Bh * (rows1 - int((s != 0).sum())), tag
        assert torch.equal(zeros, full), tag
        # through the transport front end: the same call
        o = ODE(len(tgrid), method, 4)
        via = o.sample(z, model.forward_with_cfg, cfg_table=w, slg_table=s, slg_layers=layers, cap_feats=cf, cap_mask=cm, cfg_scale=4.0, **STEP_KW)
        assert torch.equal(via, got), tag


def test_graph_path_replays_five_keys_whatever_the_tables_and_leaves_no_set(golden_dir):
    cfg, sd, (cap, cmask) = _deep(golden_dir, "next")
    model = _build("next", cfg, sd)  # a fresh engine: no key has been used
    H, W = 50, 82  # 25 x 41 = 1025 tokens: the smallest latent whose B' = 1 evaluation has more than 1024 rows
    assert (H // 2) * (W // 2) == 1025
    tgrid = ODE(7, "midpoint", 4).t  # 12 stages
    w1 = torch.tensor([2.0, 3.0, 1.0, 3.5, 1.0, 1.0, 5.0, 2.0, 1.0, 1.0, 4.0, 3.0])
    s1 = torch.tensor([2.8, 0.0, 0.0, 1.5, 2.0, 0.0, 0.0, -1.0, 3.0, 0.0, 0.0, 0.5])
    w2 = torch.tensor([1.0, 1.0, 4.5, 2.5, 2.0, 1.0, 1.0, 7.0, 3.0, 1.0, 1.0, 6.0])
    s2 = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.25, 2.0, 0.0, 4.0, 0.0, 1.0, 0.0, 3.0])
    z = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(8)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    t = torch.zeros(2, device="cuda")
    ref_cfg = model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)  # engine, weights, prompt
    ref_plain = model.forward(z, t, cap, cmask)
    model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    eng = model._engine
    layers = [1, 2]

    def kinds(w, s):  # how often each of the five keys is used: guided, cond-only, skip, guided + slg, cond + slg
        g, on = w != 1, s != 0
        return [int((g & ~on).sum()), int((~g & ~on).sum()), int(on.sum()), int((g & on).sum()), int((~g & on).sum())]

    k1, k2 = kinds(w1, s1), kinds(w2, s2)
    assert all(c > 0 for c in k1) and all(c > 0 for c in k2) and k1 != k2
    before = eng.graph_replays()
    got = model.sample_ode_cfg_schedule(z, tgrid, w1, cap, cmask, method="midpoint", return_trajectory=True, slg=s1, slg_layers=layers, **STEP_KW)
    # the first use of a key runs eagerly, every later one replays: neither scale nor the place in the tables is part of a key
    assert eng.graph_replays() - before == sum(k1) - 5
    assert eng.last_nfe() == sum(k1) and eng.last_eval_rows() == 2 * (k1[0] + k1[3]) + k1[1] + k1[2] + k1[4]
    mid = eng.graph_replays()
    other = model.sample_ode_cfg_schedule(z, tgrid, w2, cap, cmask, method="midpoint", return_trajectory=True, slg=s2, slg_layers=layers, **STEP_KW)
    assert eng.graph_replays() - mid == sum(k2)  # other table contents: the same five keys, every evaluation a replay
    again = model.sample_ode_cfg_schedule(z, tgrid, w1, cap, cmask, method="midpoint", return_trajectory=True, slg=s1, slg_layers=layers, **STEP_KW)
    assert torch.equal(again, got)
    # another set is another skip key: one eager run more
    mid = eng.graph_replays()
    model.sample_ode_cfg_schedule(z, tgrid, w1, cap, cmask, method="midpoint", slg=s1, slg_layers=[2], **STEP_KW)
    assert eng.graph_replays() - mid == sum(k1) - 1
    eng.set_option("graph", 0)
    try:
        eager = model.sample_ode_cfg_schedule(z, tgrid, w1, cap, cmask, method="midpoint", return_trajectory=True, slg=s1, slg_layers=layers, **STEP_KW)
        eager2 = model.sample_ode_cfg_schedule(z, tgrid, w2, cap, cmask, method="midpoint", return_trajectory=True, slg=s2, slg_layers=layers, **STEP_KW)
    finally:
        eng.set_option("graph", None)
    for i in range(len(tgrid)):
        assert torch.equal(got[i], eager[i]), (i, int((got[i] != eager[i]).sum()))
        assert torch.equal(other[i], eager2[i]), (i, int((other[i] != eager2[i]).sum()))
    # no set is left behind: the plain calls give what they gave before any skip call - also after a refused call
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW), ref_cfg)
    with pytest.raises(_lib.LuminaLibError, match="repeated"):
        model.sample_ode_cfg_schedule(z, tgrid, w1, cap, cmask, method="midpoint", slg=s1, slg_layers=[1, 1], **STEP_KW)
    with pytest.raises(_lib.LuminaLibError, match="outside"):
        model.forward_with_cfg_slg(z, t, cap, cmask, 4.0, slg_scale=2.0, slg_layers=[9], **STEP_KW)
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW), ref_cfg)
    assert torch.equal(model.forward(z, t, cap, cmask), ref_plain)


# ---- one evaluation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_forward_with_cfg_slg_equals_the_host_expressions(golden_dir, dtype):
    model, (cap, cmask) = _next_deep(golden_dir)
    g = torch.Generator().manual_seed(12)
    z = torch.randn(1, 4, 16, 16, generator=g).to("cuda", dtype).repeat(2, 1, 1, 1)
    t = torch.full((2,), 0.25, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    # slg_scale 0 is forward_with_cfg
    assert torch.equal(model.forward_with_cfg_slg(z, t, cap, cmask, 4.0, slg_scale=0.0, slg_layers=[1], **STEP_KW), ref)
    layers = [1, 2]
    got = model.forward_with_cfg_slg(z, t, cap, cmask, 4.0, slg_scale=2.8, slg_layers=layers, **STEP_KW)
    got1 = model.forward_with_cfg_slg(z, t, cap, cmask, 1.0, slg_scale=-1.5, slg_layers=layers, **STEP_KW)
    o = model.forward(z, t, cap, cmask).to(torch.bfloat16)
    k = model.forward(z[:1], t[:1], cap[:1].contiguous(), cmask[:1].contiguous(), skip_layers=layers).to(torch.bfloat16)
    c, u = o[:1, :3], o[1:, :3]
    gch = G.slg_combine(c, u, k[:, :3], 4.0, 2.8)
    assert torch.equal(got, torch.cat([torch.cat([gch, gch]), o[:, 3:]], 1).to(dtype))
    assert not torch.equal(got, ref)
    r = torch.cat([G.slg_combine(c, None, k[:, :3], 1.0, -1.5), o[:1, 3:]], 1)
    assert torch.equal(got1, torch.cat([r, r]).to(dtype))
    model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.forward_with_cfg_slg([z[:1], z[:1]], t, cap, cmask, 4.0, slg_scale=1.0, slg_layers=[1])


@pytest.mark.parametrize("family", ["imagenet", "flag"])
def test_other_families_run_the_same_call_through_the_transport_front_end(golden_dir, family):
    model, z, kw = _model(golden_dir, family)  # two blocks
    z = z.to("cuda", torch.bfloat16)
    assert z.shape[0] == 2
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), **kw)  # the flags a plain forward reads
    o = ODE(5, "midpoint", 4)
    w = torch.tensor([1.0, 2.0, 2.0, 1.0, 4.0, 3.0, 3.0, 1.0])
    s = torch.tensor([0.0, 2.8, 0.0, 1.5, 0.0, -1.0, 2.0, 0.0])
    nfe, rows = _counts(w, s)
    for layers in ([1], [0]):
        got = o.sample(z, model.forward_with_cfg, cfg_table=w, slg_table=s, slg_layers=layers, **kw)
        assert model._engine.last_nfe() == nfe and model._engine.last_eval_rows() == rows
        o.use_engine = False
        want = o.sample(z, model.forward_with_cfg, cfg_table=w, slg_table=s, slg_layers=layers, **kw)
        o.use_engine = True
        assert got.shape == (5,) + tuple(z.shape) and bool(torch.isfinite(want.float()).all())
        for i in range(5):
            assert torch.equal(got[i], want[i]), (family, layers, i, int((got[i] != want[i]).sum()))
    with pytest.raises(ValueError, match="rescale / norm_limit"):
        o.sample(z, model.forward_with_cfg, cfg_table=w, slg_table=s, slg_layers=[1], cfg_rescale=0.5, **kw)
    with pytest.raises(ValueError, match="guidance reuse"):
        o.sample(z, model.forward_with_cfg, cfg_table=w, slg_table=s, slg_layers=[1], cfg_reuse=[0] * 8, **kw)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    cfg, sd, (cap, cmask) = _deep(golden_dir, "next")
    model = _build("next", cfg, sd)
    n = 2 * 4 * 16 * 16
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    lim = model.engine_limits  # room for a batch of 3: the odd batch must reach its own refusal
    model.engine_limits = EngineLimits(max(lim.max_batch, 6), lim.max_tokens, lim.max_text)
    t = torch.full((2,), 0.5, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0)  # engine, weights, a prompt of 2 rows
    eng, L = model._engine, lib()
    out = torch.full((8 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    grid = (C.c_float * 4)(0.0, 0.25, 0.5, 1.0)
    f3, i32 = C.c_float * 3, C.c_int32
    good, bad = f3(4.0, 1.0, 3.0), f3(4.0, float("nan"), 3.0)
    sgood, sbad = f3(2.0, 1.5, 0.0), f3(2.0, float("inf"), 0.0)

    def call(*, tab=good, slg=sgood, skip=(1, 2), method=0, ng=4, batch=2, zz=P(z), n_skip=None, null_skip=False):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        arr = None if null_skip else (i32 * max(len(skip), 1))(*skip)
        return L.lt_sample_ode_cfg_slg(eng.handle, zz, P(out), P(out[4 * n:]), grid, ng, method, tab, slg, arr, len(skip) if n_skip is None else n_skip,
                                       1, C.byref(a), stream())

    def fwd(*, w=4.0, s=2.0, skip=(1, 2), batch=2):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        arr = (i32 * max(len(skip), 1))(*skip)
        return L.lt_forward_cfg_slg(eng.handle, P(z), P(t), P(out), w, s, arr, len(skip), C.byref(a), stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    who = "lt_sample_ode_cfg_slg:"
    # everything lt_sample_ode_cfg_schedule refuses
    refused(call(batch=3), who, "even batch")
    refused(call(tab=bad), who, "not finite")
    refused(call(ng=1), who, "2 grid points")
    refused(call(tab=None), who, "null argument")
    refused(call(zz=C.c_void_p(0)), who, "null argument")
    refused(call(method=7), who, "unknown method")
    refused(call(method=_lib.LT_ODE_ABM2), who, "unknown method")
    refused(call(batch=0), "batch 0 outside")
    refused(call(batch=4), who, "lt_prepare_prompt was called for batch 2")  # conditioning prepared for another batch
    # the slg table
    refused(call(slg=None), who, "null argument", "slg_host")
    refused(call(slg=sbad), who, "skip-layer scale of stage 0 of interval 1", "not finite")
    # the set
    refused(call(skip=(4,)), who, "skip index 4", "outside 0..3")
    refused(call(skip=(1, -1)), who, "skip index -1", "outside 0..3")
    refused(call(skip=(2, 1, 2)), who, "skip index 2 is repeated")
    refused(call(skip=(0, 1, 2, 3)), who, "leaves no layer")
    refused(call(skip=(0, 1, 2, 3, 1)), who, "5 skip indices", "4 layers")
    refused(call(n_skip=-1), who, "negative")
    refused(call(null_skip=True, n_skip=2), who, "null argument", "skip_host")
    who1 = "lt_forward_cfg_slg:"
    refused(fwd(batch=3), who1, "even batch")
    refused(fwd(w=float("nan")), who1, "not finite")
    refused(fwd(s=float("inf")), who1, "skip-layer scale is not finite")
    refused(fwd(skip=(7,)), who1, "outside 0..3")
    refused(fwd(skip=(1, 1)), who1, "repeated")
    refused(fwd(skip=(3, 2, 1, 0)), who1, "leaves no layer")
    refused(fwd(s=0.0, skip=(9,)), who1, "outside 0..3")  # also where the scale switches the skip evaluation off
    # a stream under capture: refused before anything is launched, the caller's capture stays valid and its other content replays
    a = torch.arange(64, dtype=torch.float32, device="cuda")
    graph, side, seen = torch.cuda.CUDAGraph(), torch.cuda.Stream(), []
    with torch.cuda.graph(graph, stream=side):
        seen.append((call(), L.lt_last_error().decode()))
        seen.append((fwd(), L.lt_last_error().decode()))
        arr = (i32 * 1)(1)
        sa = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        seen.append((L.lt_forward_skip(eng.handle, P(z), P(t), P(out), C.byref(sa), arr, 1, stream()), L.lt_last_error().decode()))
        b = a + 1.0
    for (rc, msg), name in zip(seen, (who, who1, "lt_forward_skip:")):
        assert rc != 0 and name in msg and "capture" in msg, (rc, msg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(b, a + 1.0) and bool(torch.isnan(out).all())
    eng.prepare_prompt_regional(cap, cmask, cap[:1].contiguous(), cmask[:1].contiguous(), 1, 1)
    refused(call(), who, "regional prompt")
    refused(fwd(), who1, "regional prompt")
    # the Python layer: what is out of scope, by name
    with pytest.raises(_lib.LuminaLibError, match="entries"):
        eng.sample_ode_cfg_slg(z, [0.0, 0.5, 1.0], [4.0, 4.0], [1.0], [1], "euler")
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        eng.sample_ode_cfg_slg([z[:1], z[:1]], [0.0, 0.5, 1.0], [4.0, 4.0], [1.0, 1.0], [1], "euler")
    with pytest.raises(_lib.LuminaLibError, match="fixed-grid"):
        eng.sample_ode_cfg_slg(z, [0.0, 0.5, 1.0], [4.0, 4.0], [1.0, 1.0], [1], "abm2")
    with pytest.raises(_lib.LuminaLibError, match="rescale / norm_limit"):
        model.sample_ode_cfg_schedule(z, [0.0, 0.5, 1.0], [4.0, 4.0], cap, cmask, method="euler", slg=[1.0, 1.0], slg_layers=[1], rescale=0.5)
    with pytest.raises(_lib.LuminaLibError, match="guidance reuse"):
        model.sample_ode_cfg_schedule(z, [0.0, 0.5, 1.0], [4.0, 4.0], cap, cmask, method="euler", slg=[1.0, 1.0], slg_layers=[1], reuse=[0, 1])
    with pytest.raises(_lib.LuminaLibError, match="fixed-grid"):
        model.sample_ode_cfg_schedule(z, [0.0, 0.5, 1.0], [4.0, 4.0], cap, cmask, method="ab2", slg=[1.0, 1.0], slg_layers=[1])
    # ... and the same arguments untouched are served, with the prompt prepared ONCE for both rows; forward_with_cfg goes on as before
    eng.prepare_prompt(cap, cmask)
    assert call() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:4 * n].float()).all()) and eng.last_nfe() == 3 + 2 and eng.last_eval_rows() == (2 + 1) + (1 + 1) + 2
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0), ref)


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_sample_driver_with_slg_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    cfg, sd, _ = _deep(golden_dir, "next")
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_slg_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_slg_test"] = ctor
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
    hi = float(tgrid[2])
    runs = {}
    try:
        for name, extra in (("default", []), ("off", ["--slg_layers", "1", "2"]), ("slg", ["--slg_layers", "1", "2", "--slg_scale", "2.8"]),
                            ("interval", ["--slg_layers", "1", "2", "--slg_scale", "2.8", "--slg_interval", "0", str(hi), "--cfg_interval", "0.1",
                                          "0.8"])):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            runs[name] = (built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
        with pytest.raises(SystemExit, match="cfg_rescale"):
            S.run(S.build_parser().parse_args(argv + ["--slg_layers", "1", "--slg_scale", "2", "--cfg_rescale", "0.5", "--image_save_path",
                                                      str(tmp_path / "no")]), encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
    finally:
        del models.__dict__["NextDiT_tiny_slg_test"]
    itab = G.cfg_table(tgrid, "midpoint", 4.0, interval=(0.1, 0.8))
    isl = G.slg_table(tgrid, "midpoint", 2.8, interval=(0.0, hi))
    nfe_i, rows_i = _counts(itab, isl)
    assert 0 < int((isl != 0).sum()) < 8 and int((itab == 1).sum()) > 0
    # every evaluation of a run lies in ONE whole-trajectory call
    assert runs == {"default": (8, 16), "off": (8, 16), "slg": (16, 24), "interval": (nfe_i, rows_i)}
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    feats, mask = encode(["a red cube", ""])
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    # the default invocation, and layers without a scale, are the call it was
    want = fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1]
    assert torch.equal(decoded[0], want / 0.13025) and torch.equal(decoded[1], decoded[0])
    fours = torch.full((8,), 4.0)
    want = model.sample_ode_cfg_schedule(z, tgrid, fours, feats, mask, method="midpoint", slg=[2.8] * 8, slg_layers=[1, 2], **kw)[:1]
    assert torch.equal(decoded[2], want / 0.13025) and not torch.equal(decoded[2], decoded[0])
    want = model.sample_ode_cfg_schedule(z, tgrid, itab, feats, mask, method="midpoint", slg=isl, slg_layers=[1, 2], **kw)[:1]
    assert torch.equal(decoded[3], want / 0.13025) and not torch.equal(decoded[3], decoded[0])
