"""Phase Upscale of multi-view (visual-anagram) sampling, the parts that need no GPU: the coefficient table against the reference's torch
expressions, the rounding chain the kernels implement (tests/views_upscale_ref.py) against the unmodified reference's bf16 run stored in
tests/golden/views_upscale_tiny.npz by scripts/make_views_upscale_golden.py (the reference is not imported here), the chunk-cover rule and
the view tables' inverse identity.

The chain is walked over the STORED per-stage model outputs of the reference run, not over the repo's CPU oracle model: that oracle restates
lumina_next_t2i's module, which the anagram fork does not equal bit for bit in bf16 (another softmax scale, query chunks over a flash-attention
stand-in).  What is checked is everything around the model: with the reference's outputs, the chain reproduces every model input and every
state of the reference's bf16 trajectory bit for bit."""
import json
import math
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, views
from lumina_t2x_amd.engine import anagram_chunks_cover, softmax_scale
from lumina_t2x_amd.transport.integrators import views_guided_table

import views_upscale_ref as UR

CASES = ["up_v2", "up_v3", "up_v1r", "up_part"]


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "views_upscale_tiny.npz"), allow_pickle=False)


def _bf(bits):
    return torch.from_numpy(bits.copy()).view(torch.bfloat16)


def _case(g, name):
    vnames, vargs = json.loads(str(g[f"{name}_views"]))
    torch.manual_seed(int(g[f"{name}_view_seed"]))
    vws = views.get_anagrams_views(vnames, view_args=vargs)
    z, guidance = torch.from_numpy(g[f"{name}_z"]), torch.from_numpy(g[f"{name}_guidance"])
    perm, vsign, isign = views.stack_tables(vws, z.shape[2], z.shape[3])
    assert np.array_equal(perm.numpy(), g[f"{name}_perm"]) and np.array_equal(vsign.numpy(), g[f"{name}_vsign"])
    assert np.array_equal(isign.numpy(), g[f"{name}_isign"])
    return vws, z.to(torch.bfloat16), guidance.to(torch.bfloat16)


def test_fixture_holds_the_cases_of_the_issue(g):
    assert json.loads(str(g["cases"])) == CASES and len(g["grid"]) == 4
    shapes = {n: (g[f"{n}_perm"].shape[0],) + tuple(g[f"{n}_z"].shape[2:]) for n in CASES}
    assert shapes == {"up_v2": (2, 32, 32), "up_v3": (3, 16, 16), "up_v1r": (1, 24, 32), "up_part": (2, 24, 24)}
    kw = {n: json.loads(str(g[f"{n}_kwargs"])) for n in CASES}
    assert kw["up_v2"] == dict(proportional_attn=True, base_seqlen=64, scale_factor=2.0) and not kw["up_v3"]["proportional_attn"]
    assert str(g["c_rounding"]) in ("state", "fp32")
    assert str(g["chunk_gap_result"]).startswith(("raised", "returned"))


@pytest.mark.parametrize("state_dtype", [torch.bfloat16, torch.float32])
def test_table_equals_the_reference_expressions_bit_for_bit(g, state_dtype):
    """generate.py:232-257 evaluated by torch, against both forms of the table; and what each form means for a product with a state tensor"""
    grid = [float(v) for v in g["grid"]] + [0.13, 0.37, 0.71, 0.93]
    grid = torch.tensor(sorted(set(grid)), dtype=torch.float32).tolist()  # a grid is fp32 values handed on as Python floats (generate.py:385)
    tab = {form: views_guided_table(grid, state_dtype, form) for form in ("fp32", "state")}
    assert tab["fp32"].shape == (len(grid) - 1, 2, 4) and tab["fp32"].dtype == torch.float32
    y = torch.randn(4096, generator=torch.Generator().manual_seed(1)).to(state_dtype)
    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = t1 - t0
        half_dt = 0.5 * dt
        for k, t in enumerate((t0, t0 + half_dt)):
            c = 0.5 * (1 + torch.cos(torch.pi * torch.tensor(t))).cpu()
            assert c.dtype == torch.float32 and c.dim() == 0
            ft, f1t, kc, k1c = tab["fp32"][i, k]
            assert float(ft) == float(torch.tensor(t, dtype=torch.float32)) and float(f1t) == float(torch.tensor(1 - t, dtype=torch.float32))
            assert torch.equal(kc, c) and torch.equal(k1c, 1 - c)
            sft, sf1t, skc, sk1c = tab["state"][i, k]
            assert torch.equal(sft, ft) and torch.equal(sf1t, f1t)
            assert torch.equal(skc, c.to(state_dtype).float()) and torch.equal(sk1c, (1 - c).to(state_dtype).float())
            # a Python float times a state tensor multiplies in fp32: ft / f1t are not rounded to the state dtype
            assert torch.equal(t * y, (y.float() * ft).to(state_dtype)) and torch.equal((1 - t) * y, (y.float() * f1t).to(state_dtype))
            # a 0-dim fp32 CPU tensor times a CPU state tensor: PyTorch's CPU kernels round the scalar to the state dtype first ("state")
            assert torch.equal((1 - c) * y, (y.float() * sk1c).to(state_dtype)) and torch.equal(c * y, (y.float() * skc).to(state_dtype))
    with pytest.raises(ValueError, match="coef_rounding"):
        views_guided_table(grid, state_dtype, "bf16")


def test_the_two_coefficient_forms_differ_at_a_bf16_state():
    """(1 - c) * y with c kept in fp32 against c rounded to bf16 first, at the times the forms were compared at"""
    y = torch.randn(4096, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    for t in (0.13, 0.37, 0.71, 0.93):
        a, b = (views_guided_table([t, 1.0], torch.bfloat16, form)[0, 0] for form in ("fp32", "state"))
        assert not torch.equal(a[2:], b[2:])
        assert not torch.equal((y.float() * a[3]).to(torch.bfloat16), (y.float() * b[3]).to(torch.bfloat16)), t


def _stored(g, name):
    xs, fs = _bf(g[f"{name}_stage_in"]), _bf(g[f"{name}_stage_out"])  # [intervals, 2, V, C, H, W]
    return xs, fs, (lambda x, t, stage: fs[stage // 2, stage % 2])


@pytest.mark.parametrize("name", CASES)
def test_chain_reproduces_the_reference_bf16_run_bit_for_bit(g, name):
    vws, z, guidance = _case(g, name)
    grid = [float(v) for v in g["grid"]]
    xs, fs, fwd = _stored(g, name)
    form = str(g["c_rounding"])
    rec = []
    traj = UR.chain_loop(fwd, vws, z, guidance, z, grid, form, rec)
    want = _bf(g[f"{name}_refbf16"])
    for k, x in enumerate(rec):  # every model input of the reference run: stage k % 2 of interval k // 2, all views
        assert torch.equal(x, xs[k // 2, k % 2]), (name, k)
    assert torch.equal(traj, want)
    assert torch.equal(_bf(g[f"{name}_rest_{form}"]), want)
    # the reference's expressions typed out (what the GPU tests evaluate on the device) are the same loop on the CPU
    assert torch.equal(UR.expression_loop(fwd, vws, z, guidance, z, grid), want)


@pytest.mark.parametrize("name", CASES)
def test_the_other_coefficient_form_is_a_different_loop_on_these_inputs(g, name):
    vws, z, guidance = _case(g, name)
    grid = [float(v) for v in g["grid"]]
    xs, fs, fwd = _stored(g, name)
    other = "fp32" if str(g["c_rounding"]) == "state" else "state"
    rec = []
    UR.chain_loop(fwd, vws, z, guidance, z, grid, other, rec)
    differing = [k for k, x in enumerate(rec) if not torch.equal(x, xs[k // 2, k % 2])]
    assert differing, name
    assert torch.equal(rec[0], xs[0, 0])  # t = 0: c = 1 exactly, the two forms coincide at the first stage
    assert not torch.equal(_bf(g[f"{name}_rest_{other}"]), _bf(g[f"{name}_refbf16"]))


def test_chunk_cover_rule():
    """int(N / base + 0.99) chunks of base rows: every shape of the fixtures and of the flagship is covered; a remainder below base / 100 is not"""
    for n, base in [(256, 64), (192, 64), (144, 64), (64, 64), (1024, 256), (16384, 256), (4096, 4096), (9216, 4096), (100, 64), (65, 64)]:
        assert anagram_chunks_cover(n, base) and UR.chunks_cover(n, base), (n, base)
    for n, base in [(258, 256), (257, 256), (4097, 4096), (8200, 4096), (12300, 4096), (1025, 1024)]:
        assert not anagram_chunks_cover(n, base) and not UR.chunks_cover(n, base), (n, base)
    for base in (64, 256, 1000, 4096):
        for n in range(1, 6 * base, 7):
            rem = n % base
            if rem and abs(rem / base - 0.01) < 1e-9:
                continue  # the boundary itself is decided by the rounding of the float sum
            want = rem == 0 or rem / base > 0.01
            assert anagram_chunks_cover(n, base) == want == UR.chunks_cover(n, base), (n, base)
    assert softmax_scale(256, 72, True, 64, _lib.LT_SOFTMAX_ANAGRAM) == math.log(256, 64) / math.sqrt(72)
    assert softmax_scale(256, 72, False, None, _lib.LT_SOFTMAX_ANAGRAM) == softmax_scale(256, 72, False, None)


@pytest.mark.parametrize("name, arg, h, w", [("identity", None, 8, 12), ("flip", None, 24, 32), ("rotate_cw", None, 16, 16), ("rotate_ccw", None, 16, 16),
                                             ("rotate_180", None, 24, 32), ("negate", None, 8, 12), ("patch_permute", "4", 16, 16),
                                             ("pixel_permute", None, 64, 64)])
def test_inverse_view_after_view_returns_to_the_pixel(name, arg, h, w):
    """iperm[perm[i]] = i: stage 1 of the guided gather reads f0 where the first stage wrote it"""
    torch.manual_seed(4)
    vw = views.get_anagrams_views([name], view_args=[arg])[0]
    perm, vsign, isign = views.stack_tables([vw], h, w)
    idx = torch.arange(h * w, dtype=torch.float32).view(1, h, w).repeat(4, 1, 1)
    iperm = (vw.inverse_view(idx) * isign[0].view(4, 1, 1))[0].flatten().long()
    assert torch.equal(iperm[perm[0].long()], torch.arange(h * w))
    assert torch.equal((vw.view(idx) * vsign[0].view(4, 1, 1))[0].flatten().long(), perm[0].long())


def test_new_entry_points_are_declared_and_bound():
    names = _lib.declared_symbols()
    for sym in ("lt_set_softmax_rule", "lt_sample_views_guided", "lt_op_views_guided_gather"):
        assert sym in names and sym in _lib._SIGNATURES
    assert (_lib.LT_SOFTMAX_T2I, _lib.LT_SOFTMAX_ANAGRAM) == (0, 1)
