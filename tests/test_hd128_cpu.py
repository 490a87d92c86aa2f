"""CPU: head_dim 128 (the 7B factories: dim 4096, 32 heads).  The fixtures made by scripts/make_hd128_golden.py from the unmodified reference
hold the oracle restatement at this head dim (tolerances of tests/test_oracle_golden.py for imagenet_tiny / full_imagenet600m), the
algorithmic-work model against a hand count, and the engine's refusals by name (no GPU work is issued here)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401  (import shim)
from lumina_t2x_amd import _lib
from lumina_t2x_amd.flops import ffn_hidden, flops_per_nfe
from oracle import odeint_oracle as OD
from oracle import synth
from oracle import variants_oracle as V


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"{name}.npz"), allow_pickle=False)


def test_imagenet_oracle_matches_reference_model_at_hd128(golden_dir):
    """Next-DiT-ImageNet DiT_Llama(dim=256, n_heads=2, n_layers=2, qk_norm=True): head_dim 128 through q_norm / k_norm, the 2-D RoPE
    table (32 frequencies per axis) and the attention, the checks of test_imagenet_oracle_matches_reference_model"""
    g = _load(golden_dir, "imagenet_tiny_hd128")
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    assert cfg.head_dim == 128 and cfg.family == "imagenet" and str(g["package"]) == "Next-DiT-ImageNet"
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    z, t, y = (torch.from_numpy(g[k]) for k in ("z", "t", "y"))
    tol = dict(rtol=0, atol=2e-5)
    out, hidden = V.imagenet_forward(sd, cfg, z, t, y, return_hidden=True)
    np.testing.assert_allclose(out.numpy(), g["forward"], **tol)
    np.testing.assert_allclose(torch.stack(hidden).numpy(), g["hidden"], **tol)
    np.testing.assert_allclose(V.imagenet_forward_with_cfg(sd, cfg, z, t, y, 4.0).numpy(), g["cfg4"], **tol)
    np.testing.assert_allclose(V.imagenet_forward_with_cfg(sd, cfg, z, t, y, 4.0, rope_scaling_factor=2.0, ntk_factor=1.5).numpy(),
                               g["cfg4_rope"], **tol)
    np.testing.assert_allclose(V.imagenet_forward_with_cfg(sd, cfg, z, t, y, 1.0).numpy(), g["cfg1_plain"], **tol)
    assert np.array_equal(g["cfg4"][0, :3], g["cfg4"][1, :3]) and not np.array_equal(g["cfg4"][0, 3], g["cfg4"][1, 3])
    traj = OD.sample_ode(lambda x, tv, **kw: V.imagenet_forward_with_cfg(sd, cfg, x, tv, **kw), z, 5, method="euler", y=y, cfg_scale=4.0)
    np.testing.assert_allclose(traj.numpy(), g["traj_euler"], rtol=0, atol=5e-5)


def test_full_imagenet7b_32_layers_oracle_and_bf16_yardstick_are_pinned_to_the_reference(golden_dir):
    """full_imagenet7b = DiT_Llama_7B_patch2(qk_norm=True), ALL 32 layers, dim 4096, 32 heads, ffn 11008, 256 tokens: the rules of
    test_fulldepth_oracle_is_pinned_to_the_reference and test_bf16_yardstick_is_pinned_to_the_reference_module_in_bf16"""
    g = _load(golden_dir, "full_imagenet7b")
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    assert (cfg.dim, cfg.n_heads, cfg.n_layers, cfg.head_dim, cfg.ffn_hidden, cfg.qk_norm) == (4096, 32, 32, 128, 11008, True)
    assert tuple(g["latent_hw"]) == (32, 32) and str(g["package"]) == "Next-DiT-ImageNet" and "reference module output" in str(g["pinned_by"])
    rel = lambda a, b: float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
    calls = json.loads(str(g["calls"]))
    assert calls
    for tag, _, _ in calls:
        ref, ora, fl, plain, ac = (g[f"{k}_{tag}"] for k in ("ref", "oracle", "floor", "refbf16", "refbf16ac"))
        assert ref.shape == ora.shape == fl.shape == plain.shape == ac.shape == (2, 4, 32, 32) and np.isfinite(ref).all()
        assert rel(ora, ref) < 1e-5
        f = rel(fl, ref)
        assert 5e-3 < f < 8e-2, f
        assert np.array_equal(ref[0, :3], ref[1, :3]) and np.array_equal(plain[0, :3], plain[1, :3])
        assert np.isfinite(plain).all() and np.isfinite(ac).all()
        for sl in (np.s_[:], np.s_[:, 3]):
            f, p, a = rel(fl[sl], ref[sl]), rel(plain[sl], ref[sl]), rel(ac[sl], ref[sl])
            assert abs(f - a) / a <= 0.10, (tag, f, a)
            assert abs(f - p) / p <= 0.15, (tag, f, p)


def test_flops_of_the_7b_config_against_a_hand_count():
    """DiT_Llama_7B_patch2: d = 4096, 32 layers, 32 heads (MHA), F = 256 * ceil(int(2 * 16384 / 3) / 256) = 256 * ceil(10922 / 256) = 11008.
    Per token and layer, in multiply-adds: wq, wk, wv, wo 4 * 4096^2 = 67 108 864; w1, w2, w3 3 * 4096 * 11008 = 135 266 304; QK^T + PV
    over N keys 2 * N * 4096.  Per sample and layer: the adaLN GEMV min(4096, 1024) * 4 * 4096 = 16 777 216.  Per token: patch embed
    16 * 4096 + final linear 4096 * 32 = 196 608.  x 2 flops, x 2 samples (the CFG pair).  head_dim 128 pads nothing: 8 k-steps of 16,
    4 blocks of 32 - the attention term is the executed MFMA work as well."""
    assert ffn_hidden(4096) == 11008 == 172 * 64
    for n in (256, 1024):
        per_tok_layer = 67108864 + 135266304 + 2 * n * 4096
        macs = 2 * (32 * (n * per_tok_layer + 16777216) + n * 196608)
        got = flops_per_nfe(dim=4096, n_layers=32, n_heads=32, n_tokens=n, batch=2)
        assert got == 2.0 * macs, (n, got, 2.0 * macs)
    # 256 tokens: 6.77 TFLOP per NFE, of which attention (4 * N^2 * d per sample and layer) is 1 %
    total = flops_per_nfe(dim=4096, n_layers=32, n_heads=32, n_tokens=256, batch=2)
    attn = 2 * 32 * 4.0 * 256 * 256 * 4096
    assert 6.7e12 < total < 6.85e12 and 0.009 < attn / total < 0.011


def _cfg(variant, **kw):
    base = dict(variant=variant, dim=256, n_layers=1, n_heads=2, n_kv_heads=2, ffn_hidden=768, patch_size=2, in_channels=4, out_channels=8,
                cap_feat_dim=128, adaln_dim=256, qk_norm=1, num_classes=10, norm_eps=1e-5, max_batch=2, max_tokens=64, max_text=64,
                rope_table_len=384)
    base.update(kw)
    return _lib.LtConfig(**base)


@pytest.mark.parametrize("variant", [_lib.LT_VARIANT_NEXT_T2I, _lib.LT_VARIANT_FLAG_T2I])
def test_text_variants_at_head_dim_128_are_refused_by_name(variant):
    """no reference factory pairs head_dim 128 with a text branch: lt_create says so before it allocates anything"""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    handle = C.c_void_p()
    assert lib.lt_create(C.byref(_cfg(variant)), C.byref(handle)) != 0
    assert b"head_dim 128 with text cross-attention not built" in lib.lt_last_error()
    assert lib.lt_create(C.byref(_cfg(variant, dim=320)), C.byref(handle)) != 0  # head_dim 160
    assert b"not built (48, 72, 96, 128)" in lib.lt_last_error()


def test_attention_describe_names_the_head_dim_128_kernels():
    """the dispatch of lt_op_attention at head_dim 128, as the library states it (host logic only): whole 64-key tiles without a key
    bias run the whole-tile kernel, everything else the general one"""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()

    def name(has_bias, acc, B, H, Hkv, N, Nk, hd):
        buf = C.create_string_buffer(64)
        assert lib.lt_op_attention_describe(has_bias, acc, B, H, Hkv, N, Nk, (Nk + 63) // 64 * 64, hd, buf, 64) == 0
        return buf.value.decode()

    for shape in [(1, 8, 8, 128), (1, 3, 3, 64), (2, 32, 32, 256), (2, 32, 32, 1024), (1, 32, 8, 4096), (2, 8, 2, 320)]:
        B, H, Hkv, N = shape
        assert name(0, 0, B, H, Hkv, N, N, 128) == "attn_fwd_kernel_hd128", shape
        assert name(1, 0, B, H, Hkv, N, N, 128) == "attn_fwd_kernel<128>", shape
        assert name(0, 1, B, H, Hkv, N, N, 128) == "attn_fwd_kernel<128>", shape
    for shape in [(1, 2, 2, 40), (1, 4, 4, 1000), (2, 8, 2, 321)]:
        B, H, Hkv, N = shape
        assert name(0, 0, B, H, Hkv, N, N, 128) == "attn_fwd_kernel<128>", shape
    assert name(0, 0, 2, 32, 32, 4096, 4096, 96) == "attn_fwd_kernel_v4h96" and name(0, 0, 2, 32, 32, 4096, 4096, 72) == "attn_fwd_kernel_v4<72>"
    assert name(0, 0, 1, 8, 8, 128, 128, 64) == "none"
