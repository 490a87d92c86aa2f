"""-m gpu: composed guidance inside the engine - lt_op_compose_* / lt_forward_compose / lt_sample_ode_compose.

The reference has no such sampler; the pin is the host definition of plain torch expressions (transport/guidance.py: guided_compose,
sample_cfg_compose) around the same engine-backed model's plain forward:

* both op entries against an exact copy and ``guided_compose``, every output word compared as an integer and the guard words behind (and, for
  the misaligned buffer, before) the outputs still NaN: all three group widths (H W = 0 mod 4, 2 mod 4, odd), a buffer misaligned by one
  element, bf16 and fp32 io, K = 1, 3, 7, on exact and on random operands, more than one block each;
* K = 1: lt_forward_compose is the first B' rows of lt_forward_cfg and lt_sample_ode_compose the first half of lt_sample_ode(use_cfg = 1)
  at every slot, word for word;
* K = 2, 3 with B' = 1, 2, distinct prompts, a table that varies per stage and a negative weight: the call equals sample_cfg_compose around
  model.forward bit for bit at every slot, on nextdit_tiny (16 x 16), nextdit_tiny_rect (16 x 24) and, with labels, imagenet_tiny;
* a plain lt_sample_ode is what it was before and after a composed call, the composed evaluations replay the graph of the lt_forward of
  (K + 1) B' rows and create no key, and the counters follow the formulas;
* every refusal by name with the NaN-filled outputs untouched;  the sample driver end to end.

Not provoked: the refusal of a layer-skip / perturb set - such a set exists only inside an lt_forward_skip / _perturb / guided-slg call."""
import ctypes as C
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

import exact_compose as X
from gpu_util import P, lib, stream
from test_gpu_sde import _model
from test_gpu_tiled import STEP, _next

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
METHODS = ["euler", "midpoint", "rk4"]
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
GUARD = 16
# H W and the elements the buffers are shifted by: group widths 4, 2, 1, and 1 again for the width-4 size on a misaligned buffer
OP_SHAPES = {"hw256_g4": (256, 0), "hw386_g2": (386, 0), "hw385_g1": (385, 0), "hw256_misaligned": (256, 1)}


def _code(dtype):
    return _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32


def _guarded(n, dtype, shift):
    """a NaN-filled buffer of ``shift + n + GUARD`` elements and its view of the n elements behind the shift"""
    buf = torch.full((shift + n + GUARD,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[shift:shift + n]


def _guards_untouched(buf, n, shift):
    return bool(torch.isnan(buf[:shift].float()).all()) and bool(torch.isnan(buf[shift + n:].float()).all())


def _farr(values):
    return (C.c_float * len(values))(*values)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("shape", sorted(OP_SHAPES))
def test_op_entries_equal_the_copy_and_guided_compose_word_for_word(shape, K, dtype):
    HW, shift = OP_SHAPES[shape]
    Bp, Cc, L = 2, 4, lib()
    n = Bp * Cc * HW
    assert n // 4 > 256  # more than one block at every group width
    # replicate: K + 1 exact copies, nothing else written
    y = torch.randn(n + shift, generator=torch.Generator().manual_seed(2)).to("cuda", dtype)[shift:]
    buf, rows = _guarded((K + 1) * n, dtype, shift)
    _lib.check(L.lt_op_compose_replicate(P(y), P(rows), K, Bp, Cc, HW, _code(dtype), stream()), "lt_op_compose_replicate")
    assert torch.equal(X.words(rows), X.words(y.repeat(K + 1))) and _guards_untouched(buf, (K + 1) * n, shift)
    for kind, ch in (("exact", 3), ("random", 3), ("random", 4), ("random", 1)):
        outs, w = (X.exact_outs if kind == "exact" else X.random_outs)(K, Bp, Cc, 1, HW, dtype, seed=11 + K)
        fbuf = torch.empty(shift + outs.numel(), dtype=dtype, device="cuda")
        f = fbuf[shift:]
        f.copy_(outs.reshape(-1))
        obuf, out = _guarded(n, dtype, shift)
        _lib.check(L.lt_op_compose_guidance(P(f), P(out), _farr(w), K, Bp, Cc, HW, ch, _code(dtype), stream()), "lt_op_compose_guidance")
        want = G.guided_compose(outs, w, ch)
        diff = X.words(out) != X.words(want.reshape(-1))
        assert not bool(diff.any()), (shape, K, kind, ch, int(diff.sum()))
        assert _guards_untouched(obuf, n, shift)
        if kind == "exact":
            assert torch.equal(X.words(want), X.words(X.compose64(outs, w, ch, exact=True)))


def test_op_entries_refuse_by_name():
    L = lib()
    f = torch.zeros(3 * 64, dtype=torch.bfloat16, device="cuda")
    out = torch.full((64,), float("nan"), dtype=torch.bfloat16, device="cuda")
    w = _farr([1.0, 1.0])

    def guidance(fp=P(f), op=P(out), wp=w, K=2, Bp=1, Cc=4, HW=16, ch=3, dt=_lib.LT_BF16):
        return L.lt_op_compose_guidance(fp, op, wp, K, Bp, Cc, HW, ch, dt, stream())

    cases = ((lambda: guidance(fp=None), "null argument"), (lambda: guidance(wp=None), "null argument"),
             (lambda: guidance(K=0), "K = 0 prompts (1 .. 7)"), (lambda: guidance(K=8), "K = 8 prompts"), (lambda: guidance(Bp=0), "B' = 0"),
             (lambda: guidance(ch=0), "cfg_channels 0 outside 1..4"), (lambda: guidance(ch=5), "cfg_channels 5"),
             (lambda: guidance(dt=_lib.LT_F16), "state dtype"),
             (lambda: guidance(wp=_farr([1.0, float("inf")])), "weight of prompt 1 is not finite"),
             (lambda: guidance(op=P(f[64:])), "out lies inside the evaluation's 3 row groups"),
             (lambda: L.lt_op_compose_replicate(None, P(f), 2, 1, 4, 16, _lib.LT_BF16, stream()), "null argument"),
             (lambda: L.lt_op_compose_replicate(P(f[64:]), P(f), 2, 1, 4, 16, _lib.LT_BF16, stream()), "y lies inside the 3 row groups"),
             (lambda: L.lt_op_compose_replicate(P(out), P(f), 9, 1, 4, 16, _lib.LT_BF16, stream()), "K = 9 prompts"))
    for call, needle in cases:
        rc = call()
        msg = L.lt_last_error().decode()
        assert rc != 0 and needle in msg and msg.startswith("compose_"), (needle, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and not bool(f.any())


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
def _tgrid(method):
    return ODE(4, method, 4).t


def _varying_table(tgrid, method, weights):
    """a table that differs from stage to stage: prompt 2 weighs 0 outside [0, 0.3), and the first stage's first weight is another"""
    table = G.compose_table(tgrid, method, weights, [None, (0.0, 0.3)] + [None] * (len(weights) - 2))
    table[0, 0] = 3.0
    assert len({tuple(r) for r in table.tolist()}) >= 3 and float(table.min()) < 0
    return table


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("Bp", [1, 2])
def test_one_prompt_is_the_first_rows_of_lt_forward_cfg(golden_dir, Bp, dtype):
    model, cap, mask = _next(golden_dir, rows=2 * Bp)
    x = torch.randn(Bp, 4, 16, 16, generator=torch.Generator().manual_seed(1)).to("cuda", dtype)
    t = torch.full((2 * Bp,), 0.3, device="cuda")
    flags = dict(STEP, scale_factor=1.0, scale_watershed=1.0)
    got = model.forward_with_compose(x, t, cap, mask, weights=[4.0], **flags)
    want = model.forward_with_cfg(x.repeat(2, 1, 1, 1), t, cap, mask, 4.0, **flags)
    assert got.dtype == dtype and bool(torch.isfinite(want.float()).all())
    assert torch.equal(X.words(got), X.words(want[:Bp]))
    assert not torch.equal(got[:, :3], model.forward_with_compose(x, t, cap, mask, weights=[1.0], **flags)[:, :3])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", METHODS)
def test_one_prompt_trajectory_is_the_first_half_of_lt_sample_ode(golden_dir, method, dtype):
    model, cap, mask = _next(golden_dir, rows=4)
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(2)).to("cuda", dtype)
    tgrid = _tgrid(method)
    flags = dict(STEP, scale_factor=1.0, scale_watershed=1.0)
    got = model.sample_ode_compose(z, tgrid, G.compose_table(tgrid, method, [4.0]), cap, mask, method=method, return_trajectory=True, **flags)
    eng = model._engine
    assert eng.last_nfe() == 3 * STAGES[method] and eng.last_eval_rows() == 4 * 3 * STAGES[method]
    want = model._engine_sample_ode(z.repeat(2, 1, 1, 1), tgrid, method, True, True, dict(cap_feats=cap, cap_mask=mask, cfg_scale=4.0, **flags))
    assert tuple(got.shape) == (4, 2, 4, 16, 16) and got.dtype == dtype and bool(torch.isfinite(want.float()).all())
    for i in range(4):
        assert torch.equal(X.words(got[i]), X.words(want[i, :2])), (method, i)
    assert torch.equal(model.sample_ode_compose(z, tgrid, G.compose_table(tgrid, method, [4.0]), cap, mask, method=method, **flags), got[-1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("name,hw,K,Bp", [("nextdit_tiny", (16, 16), 2, 1), ("nextdit_tiny", (16, 16), 2, 2), ("nextdit_tiny", (16, 16), 3, 2),
                                          ("nextdit_tiny_rect", (16, 24), 3, 1), ("nextdit_tiny_rect", (16, 24), 2, 2)])
def test_several_prompts_equal_the_host_loop_bit_for_bit(golden_dir, name, hw, K, Bp, dtype):
    rows = (K + 1) * Bp
    model, cap, mask = _next(golden_dir, name, rows=rows)
    assert len({tuple(r) for r in cap[:, 0, :4].float().tolist()}) == rows  # distinct prompts
    z = torch.randn(Bp, 4, *hw, generator=torch.Generator().manual_seed(3)).to("cuda", dtype)
    weights = [4.0, -1.5, 0.75][:K]
    t = torch.full((rows,), 0.3, device="cuda")
    v = model.forward_with_compose(z, t, cap, mask, weights=weights, **STEP)
    want_v = G.guided_compose(model.forward(z.repeat(K + 1, 1, 1, 1), t, cap, mask), weights, 3)
    assert bool(torch.isfinite(want_v.float()).all()) and torch.equal(X.words(v), X.words(want_v))
    for method in METHODS if (name, K, Bp) == ("nextdit_tiny", 2, 1) else ["midpoint"]:
        tgrid = _tgrid(method)
        table = _varying_table(tgrid, method, weights)
        got = model.sample_ode_compose(z, tgrid, table, cap, mask, method=method, return_trajectory=True, **STEP)
        eng = model._engine
        assert eng.last_nfe() == 3 * STAGES[method] and eng.last_eval_rows() == rows * 3 * STAGES[method]
        want = G.sample_cfg_compose(model.forward, z, tgrid, table, K, method, cap_feats=cap, cap_mask=mask)
        assert got.shape == want.shape == (4, Bp, 4) + hw and got.dtype == dtype
        for i in range(4):
            assert torch.equal(X.words(got[i]), X.words(want[i])), (method, i, int((got[i] != want[i]).sum()))
        # through the transport front end: the same call, and the host loop with use_engine = False
        o = ODE(4, method, 4)
        kw = dict(cap_feats=cap, cap_mask=mask, cfg_scale=4.0, **STEP)
        assert torch.equal(o.sample(z, model.forward_with_cfg, compose=table, **kw), got)
        o.use_engine = False
        assert torch.equal(o.sample(z, model.forward_with_cfg, compose=table, cap_feats=cap, cap_mask=mask), got)
    # the prompts and the order of the rows matter
    perm = [Bp + i for i in range(Bp)] + list(range(Bp)) + list(range(2 * Bp, rows))
    assert not torch.equal(model.forward_with_compose(z, t, cap[perm], mask[perm], weights=weights, **STEP), v)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_class_labels_equal_the_host_loop(golden_dir, dtype):
    model, _, _ = _model(golden_dir, "imagenet")
    K, Bp = 3, 2
    y = torch.tensor([3, 7, 1, 4, 9, 2, 10, 10], device="cuda")  # three classes per image, then the null class
    z = torch.randn(Bp, 4, 16, 16, generator=torch.Generator().manual_seed(5)).to("cuda", dtype)
    tgrid = _tgrid("midpoint")
    table = _varying_table(tgrid, "midpoint", [4.0, -1.5, 0.75])
    got = model.sample_ode_compose(z, tgrid, table, y, method="midpoint", return_trajectory=True)
    want = G.sample_cfg_compose(model.forward, z, tgrid, table, K, "midpoint", y=y)
    assert bool(torch.isfinite(want.float()).all()) and torch.equal(X.words(got), X.words(want))
    assert model._engine.last_nfe() == 6 and model._engine.last_eval_rows() == 48
    t = torch.full((8,), 0.6, device="cuda")
    assert torch.equal(X.words(model.forward_with_compose(z, t, y, weights=[4.0, -1.5, 0.75])),
                       X.words(G.guided_compose(model.forward(z.repeat(4, 1, 1, 1), t, y), [4.0, -1.5, 0.75], 3)))


def test_plain_calls_around_a_composed_call_and_no_new_graph_key(golden_dir):
    K, Bp = 2, 1
    model, cap, mask = _next(golden_dir, rows=3)
    z = torch.randn(Bp, 4, 16, 16, generator=torch.Generator().manual_seed(6)).to("cuda", torch.bfloat16)
    zp = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(7)).to("cuda", torch.bfloat16)
    tgrid = _tgrid("rk4")
    table = _varying_table(tgrid, "rk4", [4.0, -1.5])
    pkw = dict(cap_feats=cap[[0, 2]], cap_mask=mask[[0, 2]], cfg_scale=4.0, **STEP)
    t = torch.full((3,), 0.3, device="cuda")
    model.forward_with_compose(z, t, cap, mask, weights=[4.0, -1.5], **STEP)  # (the engine of every call below exists, the flags are left)
    eng = model._engine
    eng.set_option("graph", 1)  # replay at every size
    try:
        before = model._engine_sample_ode(zp, tgrid, "rk4", True, True, dict(pkw))
        rows3 = z.repeat(3, 1, 1, 1)
        plain = [model.forward(rows3, t, cap, mask) for _ in range(3)]  # the key of an lt_forward of 3 rows: run, recorded, replayed
        r0 = eng.graph_replays()
        got = model.sample_ode_compose(z, tgrid, table, cap, mask, method="rk4", return_trajectory=True, **STEP)
        # every one of the 12 evaluations replayed that key's graph: a key of the call's own would have run its first evaluation eagerly
        assert eng.graph_replays() - r0 == 12 == eng.last_nfe() and eng.last_eval_rows() == 36
        assert torch.equal(model.forward(rows3, t, cap, mask), plain[0]) and eng.graph_replays() - r0 == 13
        after = model._engine_sample_ode(zp, tgrid, "rk4", True, True, dict(pkw))
        assert eng.last_nfe() == 12 and eng.last_eval_rows() == 24
        assert model._engine is eng and torch.equal(X.words(before), X.words(after))
        want = G.sample_cfg_compose(model.forward, z, tgrid, table, K, "rk4", cap_feats=cap, cap_mask=mask)
        assert torch.equal(X.words(got), X.words(want))
    finally:
        eng.set_option("graph", None)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    model, cap, mask = _next(golden_dir, rows=3)
    lim = model.engine_limits  # room for 8 rows: a batch of 6 must reach the prompt's refusal, one of 9 the batch's
    model.engine_limits = EngineLimits(max(lim.max_batch, 8), max(lim.max_tokens, 64), max(lim.max_text, cap.shape[1]))
    x = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to("cuda", torch.bfloat16)
    n = x.numel()
    t = torch.full((8,), 0.3, device="cuda")
    model.forward_with_compose(x, t[:3], cap, mask, weights=[4.0, -1.5], **STEP)  # engine, weights, a prompt of 3 rows
    eng, L = model._engine, lib()
    mb = eng.limits.max_batch
    out = torch.full((4 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    grid = _farr([0.0, 0.25, 0.5, 1.0])
    good, bad = _farr([4.0, -1.5] * 3), _farr([4.0, -1.5, 4.0, float("nan"), 4.0, -1.5])

    def step(batch=3, h=16, ch=3, io=_lib.LT_BF16):
        a = eng._step_args(x, 1.0, 1.0, 1.0, 16, True, cfg_channels=ch)
        a.batch, a.latent_h, a.io_dtype = batch, h, io
        return a

    def sample(*, zz=P(x), g=grid, w=good, K=2, ng=4, method=0, **kw):
        return L.lt_sample_ode_compose(eng.handle, zz, P(out), P(out[3 * n:]), g, ng, method, w, K, 1, C.byref(step(**kw)), stream())

    def forward(*, xx=P(x), tt=P(t), oo=P(out), w=good, K=2, **kw):
        return L.lt_forward_compose(eng.handle, xx, tt, oo, w, K, C.byref(step(**kw)), stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    null = C.c_void_p(0)
    for who, call in (("lt_sample_ode_compose:", sample), ("lt_forward_compose:", forward)):
        refused(call(w=None), who, "null argument")
        for K in (0, -1, 8):
            refused(call(K=K), who, f"K = {K} prompts (1 .. 7)")
        for b in (4, 0, -3, 2):
            refused(call(batch=b), who, "positive multiple of K + 1 = 3")
        refused(call(batch=3 * (mb // 3 + 1)), who, f"outside 1..max_batch {mb}")
        refused(call(w=bad), who, "weight of prompt 1 at evaluation 1 is not finite") if call is sample else \
            refused(call(w=_farr([4.0, float("inf")])), who, "weight of prompt 1 at evaluation 0 is not finite")
        refused(call(ch=0), who, "cfg_channels 0 outside 1..in_channels 4")
        refused(call(ch=5), who, "cfg_channels 5")
        refused(call(h=15), who, "multiple of the patch size")
        refused(call(io=_lib.LT_F16), "io_dtype")
        refused(call(batch=6), who, "lt_prepare_prompt was called for batch 3, step has batch 6")
        refused(call(K=1, batch=4), who, "lt_prepare_prompt was called for batch 3, step has batch 4")
    refused(sample(zz=null), "lt_sample_ode_compose:", "null argument")
    refused(sample(g=None), "lt_sample_ode_compose:", "null argument")
    for k in ("xx", "tt", "oo"):
        refused(forward(**{k: null}), "lt_forward_compose:", "null argument")
    refused(sample(ng=1), "lt_sample_ode_compose:", "2 grid points")
    refused(sample(method=7), "lt_sample_ode_compose:", "unknown method 7", "euler, midpoint, rk4")
    refused(sample(method=_lib.LT_ODE_AB2), "lt_sample_ode_compose:", "unknown method")
    assert L.lt_sample_ode_compose(None, P(x), None, P(out), grid, 4, 0, good, 2, 1, C.byref(step()), stream()) != 0
    assert b"lt_sample_ode_compose: null argument" in L.lt_last_error()
    # a stream under capture: refused before anything is launched, the caller's capture stays valid and its other content replays
    a = torch.arange(64, dtype=torch.float32, device="cuda")
    graph, side, seen = torch.cuda.CUDAGraph(), torch.cuda.Stream(), []
    with torch.cuda.graph(graph, stream=side):
        seen.append((sample(), L.lt_last_error().decode()))
        b = a + 1.0
    rc, msg = seen[0]
    assert rc != 0 and "lt_sample_ode_compose:" in msg and "capture" in msg, (rc, msg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(b, a + 1.0) and bool(torch.isnan(out).all())
    eng.prepare_prompt_regional(cap[:2].contiguous(), mask[:2].contiguous(), cap[:1].contiguous(), mask[:1].contiguous(), 1, 1)
    refused(sample(), "lt_sample_ode_compose:", "regional prompt")
    refused(forward(), "lt_forward_compose:", "regional prompt")
    # the Python layer
    tab = G.compose_table([0.0, 0.5, 1.0], "euler", [4.0, -1.5])
    with pytest.raises(_lib.LuminaLibError, match="fixed-grid methods"):
        model.sample_ode_compose(x, [0.0, 0.5, 1.0], tab, cap, mask, method="ab2", **STEP)
    with pytest.raises(_lib.LuminaLibError, match="packed batch"):
        model.sample_ode_compose([x[0]], [0.0, 0.5, 1.0], tab, cap, mask, **STEP)
    with pytest.raises(_lib.LuminaLibError, match=r"\(K \+ 1\) B' = 3 rows of cap_feats"):
        model.sample_ode_compose(x, [0.0, 0.5, 1.0], tab, cap[:2], mask[:2], method="euler", **STEP)
    with pytest.raises(_lib.LuminaLibError, match="the weight table has 2 rows, the grid has 4 stages"):
        model.sample_ode_compose(x, [0.0, 0.5, 1.0], tab, cap, mask, method="midpoint", **STEP)
    with pytest.raises(_lib.LuminaLibError, match=r"K = 8 prompts \(1 \.\. 7\)"):
        model.forward_with_compose(x, t[:3], cap, mask, weights=[1.0] * 8, **STEP)
    with pytest.raises(_lib.LuminaLibError, match="t has 2 entries"):
        model.forward_with_compose(x, t[:2], cap, mask, weights=[4.0, -1.5], **STEP)
    with pytest.raises(TypeError, match="conditioning"):
        model.forward_with_compose(x, t[:3], cap, mask, cap, weights=[4.0, -1.5], **STEP)
    # ... and the same arguments untouched are served
    eng.prepare_prompt(cap, mask)
    assert sample() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    want = model.sample_ode_compose(x, [0.0, 0.25, 0.5, 1.0], [[4.0, -1.5]] * 3, cap, mask, method="euler", return_trajectory=True, **STEP)
    assert torch.equal(out[:3 * n].view(3, 1, 4, 16, 16), want[:3]) and torch.equal(out[3 * n:].view(1, 4, 16, 16), want[3])


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_sample_driver_with_composed_prompts_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_compose_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_compose_test"] = ctor
    (tmp_path / "prompts.txt").write_text("a red cube\n")
    gen = torch.Generator().manual_seed(3)
    table = {c: torch.randn(16, cfg.cap_feat_dim, generator=gen) for c in ("a red cube", "a blue ball", "fog", "")}

    def encode(caps):
        feats = torch.stack([table[c] for c in caps]).to("cuda", torch.bfloat16)
        mask = torch.ones(len(caps), 16, dtype=torch.int64, device="cuda")
        mask[-1, 8:] = 0
        return feats, mask

    decoded = []

    def decode(lat):
        decoded.append(lat.clone())
        return torch.sigmoid(lat[:, :3].float())

    argv = ["--ckpt", str(ck), "--caption_path", str(tmp_path / "prompts.txt"), "--num_sampling_steps", "5", "--sampling-method", "midpoint",
            "--time_shifting_factor", "4", "--seed", "11", "--resolution", "256:128x128"]
    comp = ["--compose_prompts", "a blue ball", "fog", "--compose_weights", "4", "-1.5", "--compose_interval", "2", "0", "0.5"]
    runs = {}
    try:
        for name, extra in (("default", []), ("composed", comp)):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            runs[name] = (built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
        with pytest.raises(SystemExit, match="--compose_prompts is not served together"):
            S.run(S.build_parser().parse_args(argv + comp + ["--cfg_interval", "0.1", "0.8", "--image_save_path", str(tmp_path / "no")]),
                  encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
    finally:
        del models.__dict__["NextDiT_tiny_compose_test"]
    # every evaluation of a run lies in ONE whole-trajectory call: 4 intervals x 2 stages, of 2 rows / of K + 1 = 3 rows
    assert runs == {"default": (8, 16), "composed": (8, 24)}
    fn = Sampler(create_transport()).sample_ode(sampling_method="midpoint", num_steps=5, time_shifting_factor=4.0)
    tgrid = fn.__self__.t
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    # without --compose_prompts the driver makes the call it made
    feats, mask = encode(["a red cube", ""])
    assert torch.equal(decoded[0], fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1] / 0.13025)
    feats, mask = encode(["a blue ball", "fog", ""])
    tab = G.compose_table(tgrid, "midpoint", [4.0, -1.5], [None, (0.0, 0.5)])
    assert len({tuple(r) for r in tab.tolist()}) == 2
    want = model.sample_ode_compose(z[:1], tgrid, tab, feats, mask, method="midpoint", **kw)
    assert tuple(decoded[1].shape) == (1, 4, 16, 16) and torch.equal(decoded[1], want / 0.13025)
