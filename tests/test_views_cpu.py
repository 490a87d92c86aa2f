"""Multi-view (visual-anagram) sampling, the parts that need no GPU: the view classes against the reference's (through the tables and
outputs stored in tests/golden/views_tiny.npz by scripts/make_views_golden.py - the reference is not imported here), the ABI declarations,
and a torch restatement of the loop (visual_anagrams/generate.py:389-414, batched the way lt_sample_views batches it) against the fixture's
fp32 trajectory through the oracle model."""
import json
import os
import re

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, views
from oracle import nextdit_oracle as O
from oracle import synth


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "views_tiny.npz"), allow_pickle=False)


def _bf(bits):
    return torch.from_numpy(bits.copy()).view(torch.bfloat16)


NAMES = ["identity", "flip", "rotate_cw", "rotate_ccw", "rotate_180", "negate", "patch_permute", "pixel_permute"]


@pytest.mark.parametrize("name", NAMES)
def test_view_classes_equal_the_reference_bit_for_bit(g, name):
    arg, hw = json.loads(str(g["vt_names"]))[name]
    torch.manual_seed(int(g["vt_seed"]))  # the random views draw with torch.randperm at construction, as the reference's do
    view = views.get_anagrams_views([name], view_args=[arg])[0]
    x = torch.from_numpy(g[f"vt_{name}_x"])
    assert torch.equal(view.view(x), torch.from_numpy(g[f"vt_{name}_view"]))
    assert torch.equal(view.inverse_view(x), torch.from_numpy(g[f"vt_{name}_inv"]))
    xb = x.to(torch.bfloat16)
    assert torch.equal(view.view(xb), torch.from_numpy(g[f"vt_{name}_view"]).to(torch.bfloat16))
    # table(): the same view as data, reproduced by plain indexing
    perm, vs, isg = view.table(hw, hw)
    assert perm.dtype == torch.int32 and vs.dtype == torch.float32 and isg.dtype == torch.float32
    assert np.array_equal(perm.numpy(), g[f"vt_{name}_perm"])
    assert np.array_equal(vs.numpy(), g[f"vt_{name}_vsign"]) and np.array_equal(isg.numpy(), g[f"vt_{name}_isign"])
    iperm = torch.empty_like(perm, dtype=torch.long)
    iperm[perm.long()] = torch.arange(perm.numel())
    assert np.array_equal(iperm.numpy(), g[f"vt_{name}_iperm"])
    flat = x.reshape(4, -1)
    assert torch.equal((flat[:, perm.long()] * vs[:, None]).view_as(x), torch.from_numpy(g[f"vt_{name}_view"]))
    assert torch.equal((flat[:, iperm] * isg[:, None]).view_as(x), torch.from_numpy(g[f"vt_{name}_inv"]))


def test_negate_view_keeps_the_reference_asymmetry():
    _, vs, isg = views.NegateView().table(8, 8)
    assert vs.tolist() == [-1, -1, -1, -1] and isg.tolist() == [-1, -1, -1, 1]
    n = torch.randn(4, 8, 8)
    out = views.NegateView().inverse_view(n)
    assert torch.equal(out[:3], -n[:3]) and torch.equal(out[3], n[3])


def test_permute_view_takes_a_caller_table_and_rejects_a_non_permutation():
    perm = torch.randperm(6 * 10)
    v = views.PermuteView(perm)
    x = torch.randn(4, 6, 10)
    assert torch.equal(v.view(x), x.reshape(4, -1)[:, perm].view(4, 6, 10))
    assert torch.equal(v.inverse_view(v.view(x)), x)
    with pytest.raises(ValueError, match="not a permutation"):
        views.PermuteView(torch.tensor([0, 1, 1, 3]))
    with pytest.raises(ValueError, match="6x12"):
        v.table(6, 12)


@pytest.mark.parametrize("name, needle", [("jigsaw", "assets"), ("inner_circle", "assets"), ("square_hinge", "assets"),
                                           ("skew", "not a pixel permutation"), ("low_pass", "not a pixel permutation"),
                                           ("grayscale", "not a pixel permutation"), ("scale", "not a pixel permutation"),
                                           ("motion", "not a pixel permutation")])
def test_views_out_of_scope_are_refused_by_name_with_the_reason(name, needle):
    with pytest.raises(views.UnsupportedViewError) as ei:
        views.get_anagrams_views([name])
    assert f"'{name}'" in str(ei.value) and needle in str(ei.value)


def test_rotations_need_a_square_latent_and_unknown_names_are_errors():
    with pytest.raises(views.UnsupportedViewError, match="square"):
        views.Rotate90CWView().table(32, 48)
    views.Rotate180View().table(32, 48)
    views.FlipView().table(32, 48)
    with pytest.raises(views.UnsupportedViewError, match="unknown view 'spiral'"):
        views.get_anagrams_views(["spiral"])


def test_header_declares_and_the_binding_table_binds_the_new_calls():
    text = _lib.header_text()
    protos = dict(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    for name, nargs in (("lt_set_views", 8), ("lt_sample_views", 9), ("lt_op_views_invert", 6), ("lt_op_views_gather", 11),
                        ("lt_op_views_reduce", 11)):
        assert name in protos, name
        assert name in _lib._SIGNATURES, name
        assert len(protos[name].split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name
    assert "const lt_step_args* a" in protos["lt_sample_views"] and "perm_dev" in protos["lt_set_views"]


def batched_loop(fwd_cfg, tabs, caps, mask, z, grid, method="midpoint", dtype=torch.float32):
    """what lt_sample_views computes, in torch: per stage ONE forward_with_cfg of 2 V rows - rows 0..V-1 view_v(latent), the rest unused
    (forward_with_cfg duplicates the first half) - then the mean over the views of inverse_view_v(-increment) is subtracted.
    `tabs` = (perm [V, HW], vsign [V, C], isign [V, C]).  R() are the bf16 rounding points (identity at fp32)."""
    perm, vs, isg = tabs
    V, HW = perm.shape
    iperm = torch.empty_like(perm)
    for v in range(V):
        iperm[v, perm[v]] = torch.arange(HW)
    Cc, H, W = z.shape[1:]
    R = (lambda x: x.to(torch.bfloat16).float()) if dtype == torch.bfloat16 else (lambda x: x)
    y = z[0].float().reshape(Cc, HW)
    states = [y.clone()]
    for i in range(len(grid) - 1):
        t0, t1 = float(grid[i]), float(grid[i + 1])
        dt = t1 - t0
        half_dt = 0.5 * dt
        dt32, hdt32 = float(np.float32(dt)), float(np.float32(half_dt))
        x = torch.stack([y[:, perm[v]] * vs[v][:, None] for v in range(V)])                       # gather
        f = fwd_cfg(torch.cat([x, x]).view(2 * V, Cc, H, W).to(dtype), torch.full((2 * V,), t0), caps, mask).float().reshape(2 * V, Cc, HW)[:V]
        if method == "midpoint":
            xm = R(x + R(f * torch.tensor(hdt32)))                                               # gather, midpoint stage
            f = fwd_cfg(torch.cat([xm, xm]).view(2 * V, Cc, H, W).to(dtype), torch.full((2 * V,), t0 + half_dt), caps, mask)
            f = f.float().reshape(2 * V, Cc, HW)[:V]
        acc = torch.zeros(Cc, HW)
        for v in range(V):                                                                        # reduce: fp32 sum in view order
            acc = acc + (-R(f[v] * torch.tensor(dt32)))[:, iperm[v]] * isg[v][:, None]
        y = R(y - R(acc / V))
        states.append(y.clone())
    return torch.stack(states).view(len(grid), Cc, H, W)


def _case(g, name):
    perm = torch.from_numpy(g[f"{name}_perm"]).long()
    tabs = (perm, torch.from_numpy(g[f"{name}_vsign"]), torch.from_numpy(g[f"{name}_isign"]))
    return tabs, _bf(g[f"{name}_caps"]).float(), torch.from_numpy(g[f"{name}_mask"]), torch.from_numpy(g[f"{name}_z"])


@pytest.mark.parametrize("name", ["v2", "v3", "v1"])
def test_batched_loop_in_fp32_reproduces_the_reference_trajectory(g, name):
    """pins the row order (view prompts, then the negative prompt per view), both signs of every view and the sign of the update: the
    restated loop through the oracle model lands on the fixture's fp32 trajectory (the reference's loop driving the reference's model,
    one batch-2 call per view, each prompt pair padded to its own length)"""
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    tabs, caps, mask, z = _case(g, name)
    # the tables the fixture recorded are the ones the package's own classes give for the same names and draw
    vnames, vargs = json.loads(str(g[f"{name}_views"]))
    torch.manual_seed(int(g[f"{name}_view_seed"]))
    mine = views.stack_tables(views.get_anagrams_views(vnames, view_args=vargs), z.shape[2], z.shape[3])
    assert torch.equal(mine[0].long(), tabs[0]) and torch.equal(mine[1], tabs[1]) and torch.equal(mine[2], tabs[2])
    V = tabs[0].shape[0]
    assert caps.shape[0] == 2 * V and all(torch.equal(caps[V][mask[V].bool()], caps[V + v][mask[V + v].bool()]) for v in range(V))
    fwd = lambda x, t, c, m: O.forward_with_cfg(sd, cfg, x, t, c, m, float(g["cfg_scale"]))
    traj = batched_loop(fwd, tabs, caps, mask, z, g["grid"].tolist())
    ref = torch.from_numpy(g[f"{name}_ref"])
    assert traj.shape == ref.shape
    err = float((traj - ref).abs().max())
    rel = float((traj[-1] - ref[-1]).norm() / ref[-1].norm())
    print(f"views_tiny/{name}: batched fp32 restatement vs reference trajectory: max abs {err:.3e}, final rel-L2 {rel:.3e}")
    assert rel < 1e-5 and err < 1e-4
    # a wrong sign of the update, or a swapped view, is far outside that: the first step alone moves the latent by O(dt)
    assert float((ref[1] - ref[0]).abs().max()) > 1e-2


def test_fixture_records_how_the_reference_rounds_dt(g):
    """dt / half_dt are Python floats in generate.py:212-219; the fixture script ran the bf16 loop both ways and recorded which one the
    reference equals bit for bit.  The engine multiplies in fp32 (csrc/views.hip) - this test fails if a regenerated fixture says otherwise."""
    assert str(g["dt_rounding"]) == "fp32"
    assert str(g["model"]) in ("visual_anagrams", "lumina_next_t2i")
