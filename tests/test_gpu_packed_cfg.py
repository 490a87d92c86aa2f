"""-m gpu: classifier-free guidance and the fixed-grid ODE trajectory on a packed (variable-resolution) batch - lt_forward_cfg_packed and
lt_sample_ode_packed through NextDiT.forward_with_cfg_packed / sample_ode_packed.

Semantics: the reference's list ``forward`` (model.py:789-834) on [x_0 .. x_{B'-1}] * 2 followed by the guidance expression of
model.py:901-913 per sample; tests/golden/nextdit_tiny_packed_cfg.npz holds that composition from the unmodified reference (CPU fp32,
scripts/make_packed_cfg_golden.py).  Three images (6 rows) at latents 12x20, 16x16, 6x16 = 60, 64, 24 tokens.

"Both halves equal" is what the tensor form guarantees and what is asserted here: the guided channels [:3] of row b and row b + B' are the
same words; channel 3 is each row's own (model.py:908-913), exactly as tests/test_gpu_model.py asserts for the tensor.

Gates: TOL_CFG4 per sample; TOL_FWD on channel 3 over all rows together, which is what the tensor test's ``got[:, 3]`` is.  TOL_FWD is a
whole-output figure (1.5 x the reference's bf16-vs-fp32 error of a full forward); on one channel of one small sample it does not hold for the
reference itself: the bf16-emulating oracle (oracle.nextdit_oracle.forward_packed, bf16=True, CPU) against this fixture gives 1.5e-2 .. 2.1e-2
per channel and sample but 2.9e-2 on channel 3 of the 6x16 sample (96 words, rms 0.76 where the others have ~1.05), and 1.8e-2 (plain) /
1.9e-2 (proportional) on channel 3 over all rows.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import DiTEngine
from oracle import odeint_oracle as OD
from oracle import synth

from gpu_util import P, rel_l2, stream
from test_gpu_model import TOL_CFG4, TOL_FWD  # the gates of the tensor forward_with_cfg golden test: imported, not restated

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
_CACHE = {}


def _case(golden_dir):
    """fixture arrays, config and ONE model for the module (the engine behind it is reused by every test)"""
    if "g" not in _CACHE:
        g = np.load(os.path.join(golden_dir, "nextdit_tiny_packed_cfg.npz"), allow_pickle=False)
        cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
        m = models.NextDiT(**cfg.ctor_kwargs())
        m.load_state_dict(synth.synth_state_dict(cfg, seed=int(g["seed_w"])), strict=True)
        _CACHE.update(g=g, cfg=cfg, model=m.eval().to("cuda", torch.bfloat16))
    return _CACHE["g"], _CACHE["cfg"], _CACHE["model"]


def _inputs(g, dtype):
    sizes = [tuple(int(v) for v in hw) for hw in g["sizes"]]
    xs = [torch.from_numpy(g[f"x{b}"]).to("cuda", dtype) for b in range(len(sizes))]
    if "in" not in _CACHE:
        _CACHE["in"] = (torch.from_numpy(g["t"]).cuda(), torch.from_numpy(g["cap"]).to("cuda", torch.bfloat16), torch.from_numpy(g["mask"]).cuda())
    return sizes, xs + [x.clone() for x in xs], _CACHE["in"]


@pytest.mark.parametrize("prop", [False, True], ids=["plain", "prop16"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_forward_with_cfg_packed_vs_reference_composition(golden_dir, dtype, prop):
    g, cfg, model = _case(golden_dir)
    sizes, xs, (t, cap, mask) = _inputs(g, dtype)
    half = len(sizes)
    kw = dict(proportional_attn=True, base_seqlen=16) if prop else {}
    ys = model.forward_with_cfg_packed(xs, t, cap, mask, float(g["cfg_scale"]), **kw)
    assert isinstance(ys, list) and len(ys) == 2 * half
    key = "cfgprop" if prop else "cfg"
    for b, y in enumerate(ys):
        ref = torch.from_numpy(g[f"{key}{b}"])
        assert tuple(y.shape) == (cfg.in_channels,) + sizes[b % half] and y.dtype == dtype and y.is_cuda
        err = rel_l2(y, ref)
        print(f"packed cfg {key} sample {b} {sizes[b % half]}: rel-L2 {err:.3e} (gate {TOL_CFG4})")
        assert err < TOL_CFG4, (key, b, err)
    # the unguided channel over all rows (got[:, 3] of the tensor test): the network error without the guidance's amplification
    ch3, ref3 = (torch.cat([v[3].reshape(-1) for v in vs]) for vs in (ys, [torch.from_numpy(g[f"{key}{b}"]) for b in range(2 * half)]))
    err3 = rel_l2(ch3, ref3)
    print(f"packed cfg {key} channel 3, all rows: rel-L2 {err3:.3e} (gate {TOL_FWD})")
    assert err3 < TOL_FWD, (key, err3)
    for b in range(half):  # the guided channels are one result written to both rows
        assert torch.equal(ys[b][:3], ys[b + half][:3]), b
    assert len({y.untyped_storage().data_ptr() for y in ys}) == 1  # views of one allocation
    # the second half of the input is not read (combined = cat([half, half]), model.py:901-902)
    xs2 = xs[:half] + [torch.full_like(x, 123.0) for x in xs[half:]]
    for a, b in zip(model.forward_with_cfg_packed(xs2, t, cap, mask, float(g["cfg_scale"]), **kw), ys):
        assert torch.equal(a, b)


@pytest.mark.parametrize("prop", [False, True], ids=["plain", "prop16"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_equal_sizes_are_bit_identical_to_the_tensor_forward_with_cfg(golden_dir, dtype, prop):
    g, cfg, model = _case(golden_dir)
    _, _, (t, cap, mask) = _inputs(g, dtype)
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(3, cfg.in_channels, 16, 16, generator=gen).to("cuda", dtype)
    z = torch.cat([z, z])
    kw = dict(proportional_attn=True, base_seqlen=16) if prop else {}
    want = model.forward_with_cfg(z, t, cap, mask, 4.0, **kw)
    got = model.forward_with_cfg_packed(list(z), t, cap, mask, 4.0, **kw)
    for b in range(6):
        assert torch.equal(got[b], want[b]), b


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_sample_ode_packed_equals_stepwise_torch(golden_dir, dtype, method):
    """lt_sample_ode_packed (the C++ loop on the flat state) == torchdiffeq's arithmetic driven from Python over forward_with_cfg_packed, formed as
    the lt_sample_ode tests form it (oracle.odeint_oracle.odeint on the state; a list state is the cat of its samples): bit for bit."""
    g, cfg, model = _case(golden_dir)
    sizes, zs, (_, cap, mask) = _inputs(g, dtype)
    kw = dict(proportional_attn=True, base_seqlen=16)
    tgrid = OD.time_grid(4, 4)  # 3 intervals
    shapes = [tuple(z.shape) for z in zs]
    counts = [z.numel() for z in zs]

    def split(flat):
        return [p.view(s) for p, s in zip(flat.split(counts), shapes)]

    def f(tt, flat):
        tvec = torch.ones(len(zs)).to(flat.device) * tt  # integrators.py:108
        return torch.cat([o.reshape(-1) for o in model.forward_with_cfg_packed(split(flat), tvec, cap, mask, 4.0, **kw)])

    slow = OD.odeint(f, torch.cat([z.reshape(-1) for z in zs]), tgrid, method=method)
    eng = model._engine
    stages = {"euler": 1, "midpoint": 2, "rk4": 4}[method]
    results = {}
    try:
        for graph in (0, 1):
            eng.set_option("graph", graph)
            before = eng.graph_replays()
            results[graph] = model.sample_ode_packed(zs, tgrid, cap, mask, 4.0, method=method, return_trajectory=True, **kw)
            assert eng.last_nfe() == 3 * stages
            replays = eng.graph_replays() - before
            assert (replays > 0) if graph else (replays == 0), (graph, replays)
        final = model.sample_ode_packed(zs, tgrid, cap, mask, 4.0, method=method, **kw)
    finally:
        eng.set_option("graph", None)
    for b, (fast, fast_g) in enumerate(zip(results[0], results[1])):
        assert tuple(fast.shape) == (4,) + shapes[b] and fast.dtype == dtype
        want = torch.stack([split(slow[i])[b] for i in range(4)])
        assert torch.equal(fast, want), (b, float((fast.float() - want.float()).abs().max()))
        assert torch.equal(fast_g, fast), b
        assert torch.equal(final[b], fast[-1]) and tuple(final[b].shape) == shapes[b], b
    assert len({y.untyped_storage().data_ptr() for y in results[0]}) == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_lt_forward_packed_is_untouched(golden_dir, dtype):
    """the plain packed forward keeps its launches: the assertions of tests/test_gpu_model.py's packed test on the fixture nextdit_tiny_packed hold,
    "the longest sample equals its solo run, bit for bit" included - also with the flat entry points used on the same engine in between"""
    g = np.load(os.path.join(golden_dir, "nextdit_tiny_packed.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    model = models.NextDiT(**cfg.ctor_kwargs())
    model.load_state_dict(synth.synth_state_dict(cfg, seed=int(g["seed_w"])), strict=True)
    model = model.eval().to("cuda", torch.bfloat16)
    sizes = [tuple(int(v) for v in hw) for hw in g["sizes"]]
    xs = [torch.from_numpy(g[f"x{b}"]).to("cuda", dtype) for b in range(len(sizes))]
    t, cap = torch.from_numpy(g["t"]).cuda(), torch.from_numpy(g["cap"]).to("cuda", torch.bfloat16)
    mask = torch.from_numpy(g["mask"]).cuda()
    ys = model(xs, t, cap, mask)
    model.forward_with_cfg_packed([xs[0], xs[1], xs[0], xs[1]], t, cap, mask, 4.0)  # the flat entry point on the same engine, in between
    ys_again = model(xs, t, cap, mask)
    assert isinstance(ys, list) and len(ys) == len(sizes)
    for b, y in enumerate(ys):
        ref = torch.from_numpy(g[f"y{b}"])
        assert tuple(y.shape) == (cfg.in_channels,) + sizes[b] and y.dtype == dtype
        assert rel_l2(y, ref) < TOL_FWD, (b, rel_l2(y, ref))
        assert torch.equal(y, ys_again[b]), b
    solo = model(xs[0][None], t[:1], cap[:1], mask[:1])[0]
    assert torch.equal(solo, ys[0])
    for layer in model.layers:  # as forward_with_cfg leaves them (model.py:891-899)
        layer.attention.proportional_attn, layer.attention.base_seqlen = True, 16
    yp = model(xs, t, cap, mask)
    for b, y in enumerate(yp):
        ref = torch.from_numpy(g[f"yprop{b}"])
        assert rel_l2(y, ref) < TOL_FWD, (b, rel_l2(y, ref))
    short = min(range(len(sizes)), key=lambda b: sizes[b][0] * sizes[b][1])
    assert rel_l2(yp[short], torch.from_numpy(g[f"solo_prop{short}"])) > rel_l2(yp[short], torch.from_numpy(g[f"yprop{short}"]))
    with pytest.raises(TypeError):
        model.forward_with_cfg(xs, t, cap, mask, 4.0)


def _hw(sizes):
    return (C.c_int32 * (2 * len(sizes)))(*[v for s in sizes for v in s])


def test_refusals_name_the_cause_and_leave_the_output_untouched(golden_dir):
    g, cfg, model = _case(golden_dir)
    sizes, xs, (t, cap, mask) = _inputs(g, torch.bfloat16)
    model.forward_with_cfg_packed(xs, t, cap, mask, 4.0)  # the engine holds the weights and a prompt of 6 rows
    eng, L = model._engine, _lib.load()
    n = 8 * 4 * 16 * 16
    x = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    out = torch.full((4 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    t8 = torch.full((8,), 0.5, device="cuda")
    grid = (C.c_float * 3)(0.0, 0.5, 1.0)
    six = sizes + sizes

    def args(batch):
        a = eng._step_args(x.view(1, 1, 1, -1), 4.0, 1.0, 1.0, None, False)
        a.batch, a.latent_h, a.latent_w = batch, 0, 0
        return a

    def fwd(hw, batch, *, h=eng.handle, xp=P(x), tp=P(t8), op=P(out), a=True):
        ar = args(batch)
        return L.lt_forward_cfg_packed(h, xp, hw, tp, op, C.byref(ar) if a else None, stream())

    def ode(hw, batch, *, h=eng.handle, zp=P(x), gp=grid, ng=3, method=0, use_cfg=1, a=True):
        ar = args(batch)
        return L.lt_sample_ode_packed(h, zp, hw, P(out), P(out[2 * n:]), gp, ng, method, use_cfg, 1, C.byref(ar) if a else None, stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    null = C.c_void_p(0)
    for call in (fwd, ode):
        refused(call(_hw(six), 6, h=null), "null argument")
        refused(call(None, 6), "null argument")
        refused(call(_hw(six), 6, a=False), "null argument")
        refused(call(_hw(sizes), 3), "even batch")
        refused(call(_hw(sizes + sizes[::-1]), 6), "halves differ")
        refused(call(_hw([(16, 16)] * 66), 66), "max_batch")
        refused(call(_hw([(16, 16)] * 8), 8), "max_batch")
        refused(call(_hw([(16, 16), (15, 16)] * 3), 6), "multiple of the patch size")
        refused(call(_hw([(16, 16), (0, 16)] * 3), 6), "multiple of the patch size")
        refused(call(_hw([(130, 128), (16, 16), (16, 16)] * 2), 6), "max_tokens")
        refused(call(_hw([(2, 770), (16, 16), (16, 16)] * 2), 6), "RoPE table")
    refused(fwd(_hw(six), 6, xp=null), "null argument")
    refused(fwd(_hw(six), 6, tp=null), "null argument")
    refused(fwd(_hw(six), 6, op=null), "null argument")
    refused(ode(_hw(six), 6, zp=null), "null argument")
    refused(ode(_hw(six), 6, gp=None), "null argument")
    refused(ode(_hw(six), 6, method=7), "unknown method")
    refused(ode(_hw(six), 6, method=-1), "unknown method")
    refused(ode(_hw(six), 6, ng=1), "2 grid points")
    # a regional prompt on the engine
    eng.prepare_prompt_regional(cap[:2].contiguous(), mask[:2].contiguous(), cap[:1].contiguous(), mask[:1].contiguous(), 1, 1)
    for call in (fwd, ode):
        refused(call(_hw([(16, 16)] * 2), 2), "regional")
    eng.prepare_prompt(cap, mask)
    # any other variant
    other = DiTEngine(variant=_lib.LT_VARIANT_NEXT_IMAGENET, dim=576, n_layers=1, n_heads=8, n_kv_heads=8, ffn_hidden=256, patch_size=2, in_channels=4,
                      out_channels=8, cap_feat_dim=0, qk_norm=True, norm_eps=1e-5, num_classes=10)
    for call in (fwd, ode):
        refused(call(_hw(six), 6, h=other.handle), "LT_VARIANT_NEXT_T2I")
    # ... and the engine still serves the call it refused nothing of
    ys = model.forward_with_cfg_packed(xs, t, cap, mask, 4.0)
    assert all(bool(torch.isfinite(y.float()).all()) for y in ys)
