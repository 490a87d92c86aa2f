"""-m gpu: packed (variable-resolution) batches on the head_dim-72 one-wave attention kernel and in the pair-layout regime.

The one-wave kernel and the ping-pong kernel are bit-identical, so are the pair layout and the row-major one: forward_with_cfg_packed and
sample_ode_packed under the default options must give the words they give under attention_variant 3 (the ping-pong kernel, the transpose
kernels for V, row-major operands: the launches packed batches had before) and under pair_layout 0.  Sizes: the fixture of
tests/test_gpu_packed_cfg.py (60, 64, 24 tokens: one key tile, two of three samples masked), latents whose longest sequence is five tiles
(320, 300, 30 tokens), and - for the pair regime, which the engine takes from one 256-row GEMM tile per CU on - 4096, 3952 and 64 tokens
on a one-layer model of the same width.

The comparison with the reference composition (tests/golden/nextdit_tiny_packed_cfg.npz) is not repeated here: tests/test_gpu_packed_cfg.py makes it,
unchanged, and its fixture (longest sequence 64 tokens, two shorter samples) now dispatches to the per-sample key count instantiation of the one-wave
kernel under the default options - the first test below asserts that dispatch for the same sizes."""
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import models
from lumina_t2x_amd.engine import EngineLimits
from oracle import odeint_oracle as OD
from oracle import synth

import attention_nk_cases as K

pytestmark = pytest.mark.gpu

_CACHE = {}


def _tiny(golden_dir):
    if "tiny" not in _CACHE:
        g = np.load(os.path.join(golden_dir, "nextdit_tiny_packed_cfg.npz"), allow_pickle=False)
        cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
        m = models.NextDiT(**cfg.ctor_kwargs())
        m.load_state_dict(synth.synth_state_dict(cfg, seed=int(g["seed_w"])), strict=True)
        _CACHE["tiny"] = (g, cfg, m.eval().to("cuda", torch.bfloat16))
    return _CACHE["tiny"]


def _latents(sizes, channels, seed, dtype=torch.bfloat16):
    gen = torch.Generator().manual_seed(seed)
    xs = [torch.randn(channels, h, w, generator=gen).to("cuda", dtype) for h, w in sizes]
    return xs + [x.clone() for x in xs]


def _prompt(g):
    return torch.from_numpy(g["t"]).cuda(), torch.from_numpy(g["cap"]).to("cuda", torch.bfloat16), torch.from_numpy(g["mask"]).cuda()


def _with_options(eng, opts, fn):
    try:
        for n, v in opts.items():
            eng.set_option(n, v)
        return fn()
    finally:
        for n in opts:
            eng.set_option(n, None)


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and bool(torch.isfinite(x.float()).all()), (what, i)
        assert torch.equal(x, y), (what, i, int((x != y).sum()), float((x.float() - y.float()).abs().max()))


@pytest.mark.parametrize("sizes", [None, [(16, 16), (16, 12), (12, 16)], [(32, 40), (30, 40), (10, 12)]], ids=["fixture", "64_48_48", "320_300_30"])
def test_packed_cfg_and_ode_on_the_one_wave_kernel_equal_the_ping_pong_kernel(golden_dir, sizes):
    g, cfg, model = _tiny(golden_dir)
    t, cap, mask = _prompt(g)
    if sizes is None:
        sizes = [tuple(int(v) for v in hw) for hw in g["sizes"]]
        xs = [torch.from_numpy(g[f"x{b}"]).to("cuda", torch.bfloat16) for b in range(len(sizes))]
        xs = xs + [x.clone() for x in xs]
    else:
        xs = _latents(sizes, cfg.in_channels, 7)
    ntok = [(h // 2) * (w // 2) for h, w in sizes]
    N = max(ntok)
    assert N % 64 == 0 and min(ntok) < N
    H, Hkv = cfg.n_heads, cfg.n_kv_heads or cfg.n_heads
    assert K.describe(2 * len(sizes), H, Hkv, N, N, 72, has_nk=True, has_text=True, Tkpad=(cap.shape[1] + 63) // 64 * 64) == "attn_fwd_kernel_v4<72>"
    kw = dict(proportional_attn=True, base_seqlen=16)
    tgrid = OD.time_grid(4, 4)  # 3 grid intervals
    fwd = lambda: model.forward_with_cfg_packed(xs, t, cap, mask, 4.0, **kw)  # noqa: E731
    ode = lambda: model.sample_ode_packed(xs, tgrid, cap, mask, 4.0, method="euler", return_trajectory=True, **kw)  # noqa: E731
    y4, z4 = [v.clone() for v in fwd()], [v.clone() for v in ode()]
    eng = model._engine
    y3 = _with_options(eng, {"attention_variant": 3}, lambda: [v.clone() for v in fwd()])
    z3 = _with_options(eng, {"attention_variant": 3}, lambda: [v.clone() for v in ode()])
    _same(y4, y3, "forward_with_cfg_packed")
    _same(z4, z3, "sample_ode_packed")
    assert any(not torch.equal(a[0], a[-1]) for a in z4)  # the trajectory moved


def test_packed_batch_in_the_pair_regime_equals_row_major(golden_dir):
    """one layer, d = 576, 6 rows x 4096 tokens = 96 row tiles x 3 column tiles >= one per CU: the engine takes the pair layout (and the V^T
    epilogue of the fused QKV GEMM) on a packed batch; the same evaluation under pair_layout 0, and under attention_variant 3 (no pair
    layout, no V^T epilogue: the launches packed batches had before), gives the same words"""
    g, _, _ = _tiny(golden_dir)
    cfg = synth.NextDiTConfig(**dict(json.loads(str(g["config"])), n_layers=1))
    assert cfg.dim == 576 and cfg.head_dim == 72
    model = models.NextDiT(**cfg.ctor_kwargs())
    model.load_state_dict(synth.synth_state_dict(cfg, seed=5), strict=True)
    model = model.eval().to("cuda", torch.bfloat16)
    sizes = [(128, 128), (104, 152), (16, 16)]
    model.engine_limits = EngineLimits(max_batch=6, max_tokens=4096, max_text=int(g["cap"].shape[1]))
    xs = _latents(sizes, cfg.in_channels, 11)
    t, cap, mask = _prompt(g)
    kw = dict(proportional_attn=True, base_seqlen=1024)
    fwd = lambda: [v.clone() for v in model.forward_with_cfg_packed(xs, t, cap, mask, 4.0, **kw)]  # noqa: E731
    y = fwd()
    eng = model._engine
    assert eng.get_option("last_pair") == 1, "the packed evaluation did not take the pair regime"
    y0 = _with_options(eng, {"pair_layout": 0}, lambda: (fwd(), eng.get_option("last_pair")))
    assert y0[1] == 0
    _same(y, y0[0], "pair_layout 0")
    y3 = _with_options(eng, {"attention_variant": 3}, lambda: (fwd(), eng.get_option("last_pair")))
    assert y3[1] == 0
    _same(y, y3[0], "attention_variant 3")
    y1 = fwd()
    assert eng.get_option("last_pair") == 1
    _same(y, y1, "again, after the layout went back and forth")
    with pytest.raises(Exception):
        eng.set_option("last_pair", 1)  # read-only: no such option to set
