"""-m gpu: head_dim 128 (the 7B factories: dim 4096, 32 heads) - the attention kernels (whole-tile kernel attention_hd128.hip, general
path attn_fwd_kernel<128>), the operators below them at this head dim / width, and the engine against the fixtures
scripts/make_hd128_golden.py made from the unmodified reference (imagenet_tiny_hd128, full_imagenet7b)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.transport import Sampler, create_transport
from oracle import synth

import test_gpu_fulldepth as FD
import test_gpu_ops as OPS
from gpu_util import P, bf, lib, max_abs, ok, r16, rel_l2, set_option, stream
from test_gpu_variants import TOL_CFG4, TOL_FWD, _build, _golden

pytestmark = pytest.mark.gpu

HD = 128
FAST, GENERAL = "attn_fwd_kernel_hd128", "attn_fwd_kernel<128>"


@pytest.fixture(autouse=True)
def _default_kernel_variants():
    yield
    set_option("attention_variant", 4)
    set_option("gemm_variant", 0)


def _kernel(B, H, Hkv, N, bias=False, accumulate=False):
    buf = C.create_string_buffer(64)
    ok(lib().lt_op_attention_describe(int(bias), int(accumulate), B, H, Hkv, N, N, (N + 63) // 64 * 64, HD, buf, 64))
    return buf.value.decode()


def _qkv(B, H, Hkv, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (bf(torch.randn(B, H, N, HD, generator=g)), bf(torch.randn(B, Hkv, N, HD, generator=g)), bf(torch.randn(B, Hkv, N, HD, generator=g)))


SHAPES = [(1, 8, 8, 128), (2, 8, 2, 320), (1, 3, 3, 64), (1, 2, 2, 40), (2, 32, 32, 256), (2, 32, 32, 1024), (1, 32, 8, 4096), (1, 4, 4, 1000)]


@pytest.mark.parametrize("B,H,Hkv,N", SHAPES)
@pytest.mark.parametrize("fold", [False, True])
def test_attention_self_hd128(B, H, Hkv, N, fold):
    """lt_op_attention at head_dim 128 against the exact fp32 softmax, the bound of test_attention_self; whole 64-key tiles take the
    whole-tile kernel (GQA included), ragged key counts the general one - as the library's own dispatch states it"""
    assert _kernel(B, H, Hkv, N) == (FAST if N % 64 == 0 else GENERAL)
    q, k, v = _qkv(B, H, Hkv, N, N + HD)
    scale = math.sqrt(math.log(N, 64) / HD) if N > 64 else 1 / math.sqrt(HD)
    out = OPS._run_attn(q, k, v, scale, fold_scale=fold)
    ref = OPS._attn_ref(q.cpu(), k.cpu(), v.cpu(), scale)
    assert not torch.isnan(out.float()).any()
    e = rel_l2(out, ref)
    print(f"hd128 attention {(B, H, Hkv, N)} fold {fold}: rel_l2 {e:.3e} ({_kernel(B, H, Hkv, N)})")
    assert e < 6e-3, e


@pytest.mark.parametrize("B,H,Hkv,N", [(1, 8, 8, 128), (2, 32, 32, 256), (2, 32, 32, 1024), (1, 32, 8, 4096), (2, 8, 2, 320)])
def test_attention_hd128_whole_tile_kernel_against_the_general_path(B, H, Hkv, N):
    """the same whole-tile inputs through both kernels (attention_variant 1 keeps launch_attention off the whole-tile kernel): each
    within 6e-3 of fp32 and within 6e-3 of the other (different max / row-sum bookkeeping: not bit-identical by construction)"""
    q, k, v = _qkv(B, H, Hkv, N, 7 * N + 1)
    scale = 1 / math.sqrt(HD)
    ref = OPS._attn_ref(q.cpu(), k.cpu(), v.cpu(), scale)
    assert _kernel(B, H, Hkv, N) == FAST
    fast = OPS._run_attn(q, k, v, scale, fold_scale=True)
    set_option("attention_variant", 1)
    assert _kernel(B, H, Hkv, N) == GENERAL
    gen = OPS._run_attn(q, k, v, scale, fold_scale=True)
    set_option("attention_variant", 4)
    e_f, e_g, e_fg = rel_l2(fast, ref), rel_l2(gen, ref), rel_l2(fast, gen)
    print(f"hd128 {(B, H, Hkv, N)}: whole-tile vs fp32 {e_f:.3e}, general vs fp32 {e_g:.3e}, whole-tile vs general {e_fg:.3e}")
    assert e_f < 6e-3 and e_g < 6e-3 and e_fg < 6e-3, (e_f, e_g, e_fg)


@pytest.mark.parametrize("N,valid1", [(128, 40), (200, 130), (64, 64)])
def test_attention_hd128_with_a_key_bias(N, valid1):
    """a 0 / -inf key bias (the masked kernels' input) runs the general path at every key count"""
    B, H, Hkv = 2, 8, 2
    assert _kernel(B, H, Hkv, N, bias=True) == GENERAL
    q, k, v = _qkv(B, H, Hkv, N, 3 * N + valid1)
    bias = torch.zeros(B, N)
    bias[1, valid1:] = float("-inf")
    scale = 1 / math.sqrt(HD)
    for fold in (False, True):
        out = OPS._run_attn(q, k, v, scale, bias=bias, fold_scale=fold)
        ref = OPS._attn_ref(q.cpu(), k.cpu(), v.cpu(), scale, bias=bias)
        assert rel_l2(out, ref) < 6e-3, (fold, rel_l2(out, ref))


@pytest.mark.parametrize("variant", [1, 4])
def test_attention_hd128_softmax_outlier_keys(variant):
    """test_attention_softmax_outlier_keys at head_dim 128: running-max jumps mid-sequence above and below the deferred-rescale
    threshold, on the general path (rescale every tile) and the whole-tile kernel (threshold 8 in log2 units)"""
    set_option("attention_variant", variant)
    B, H, N = 1, 8, 256
    assert _kernel(B, H, H, N) == (FAST if variant == 4 else GENERAL)
    g = torch.Generator().manual_seed(9)
    q = bf(torch.randn(B, H, N, HD, generator=g))
    k = bf(torch.randn(B, H, N, HD, generator=g))
    v = bf(torch.randn(B, H, N, HD, generator=g))
    k[:, :, 131] = q[:, :, 7] * 4.0
    k[:, :, 3] = q[:, :, 200] * 2.0
    k[:, :, 70] = q[:, :, 100] * 0.35
    k[:, :, :64] -= q[:, :, 50:51] * 3.0
    out = OPS._run_attn(q, k, v, 1 / math.sqrt(HD))
    ref = OPS._attn_ref(q.cpu(), k.cpu(), v.cpu(), 1 / math.sqrt(HD))
    assert rel_l2(out, ref) < 6e-3, rel_l2(out, ref)


# ---- the operators below the attention at head_dim 128 / K = d = 4096: the checks of test_gpu_ops.py at the 7B's shapes ------------------

@pytest.mark.parametrize("heads,qk_norm", [(2, True), (32, True), (32, False)])
def test_qk_norm_rope_hd128(heads, qk_norm):
    OPS.test_qk_norm_rope(heads, HD, qk_norm)


@pytest.mark.parametrize("N,kvh", [(64, 2), (100, 8), (256, 32)])
def test_v_transpose_is_exact_hd128(N, kvh):
    OPS.test_v_transpose_is_exact(N, kvh, HD)


@pytest.mark.parametrize("tokens,B,kvh,K,variant", [(256, 2, 32, 4096, 0), (1024, 2, 32, 4096, 0), (64, 3, 2, 128, 1), (128, 2, 8, 512, 2)])
def test_gemm_vt_epilogue_hd128(tokens, B, kvh, K, variant):
    OPS.test_gemm_vt_epilogue_matches_gemm_plus_transpose(tokens, B, kvh, HD, K, variant)


@pytest.mark.parametrize("tokens,B,H,Hkv,K", [(4096, 2, 32, 32, 4096), (4096, 2, 32, 8, 4096), (1024, 8, 32, 32, 256)])
def test_gemm_fused_qkv_hd128(tokens, B, H, Hkv, K):
    """N = 3 * 4096 (MHA) / 4096 + 2 * 1024 (GQA): whole 256-wide tiles on both sides of the V split, two heads per V^T tile"""
    assert lib().lt_op_gemm_qkv_fusable(B * tokens, H * HD + 2 * Hkv * HD, K, H * HD + Hkv * HD, tokens, HD) != 0
    OPS.test_gemm_fused_qkv_matches_separate_launches(tokens, B, H, Hkv, HD, K)


def test_rmsnorm_mod_d4096():
    B, N, d = 2, 70, 4096
    g = torch.Generator().manual_seed(1)
    x = bf(torch.randn(B * N, d, generator=g) * 3)
    w = bf(1 + 0.1 * torch.randn(d, generator=g))
    ld = 3 * d
    mod = bf(torch.randn(B, ld, generator=g) * 0.5)
    out = torch.empty_like(x)
    ok(lib().lt_op_rmsnorm_mod(P(x), P(w), P(mod[:, d:]), None, ld, P(out), B, N, d, 1e-5, 0, stream()))
    torch.cuda.synchronize()
    xf = x.float().cpu()
    n = r16(xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5))
    n = r16(n * w.float().cpu())
    sc = mod.float().cpu()[:, d:2 * d].repeat_interleave(N, dim=0)
    ref = r16(n * r16(1 + sc))
    assert rel_l2(out, ref) < 2e-3, rel_l2(out, ref)
    assert max_abs(out, ref) <= 0.07


@pytest.mark.parametrize("post_mode,next_mode", [(1, 1), (1, 2), (0, 1), (0, 2)])
def test_gated_residual_norm_d4096(post_mode, next_mode):
    """d = 4096 has no compile-time-specialised row kernel (those are built for 1536 / 2304 / 3072): it runs the generic 8-chunk kernel
    with norm_specialize on or off, and that kernel holds the reference's rounding order at this width"""
    OPS.test_gated_residual_norm_specialised_is_bit_identical(4096, post_mode, next_mode)
    B, N, d = 2, 33, 4096
    g = torch.Generator().manual_seed(40 + next_mode)
    x = bf(torch.randn(B * N, d, generator=g))
    y = bf(torch.randn(B * N, d, generator=g) * 2)
    pw, nw = bf(1 + 0.1 * torch.randn(d, generator=g)), bf(1 + 0.1 * torch.randn(d, generator=g))
    ld = 4 * d
    mod = bf(torch.randn(B, ld, generator=g))
    xs, h = x.clone(), torch.full_like(x, float("nan"))
    ok(lib().lt_op_gated_residual_norm(P(xs), P(y), P(pw), P(mod[:, d:]), 1, 1, P(nw) if next_mode == 1 else None, P(mod[:, 2 * d:]), None, next_mode,
                                       ld, P(h), B, N, d, 1e-5, 1e-6, 0, stream()))
    torch.cuda.synchronize()
    m = mod.float().cpu()
    gate = r16(torch.tanh(m[:, d:2 * d])).repeat_interleave(N, dim=0)
    scale = m[:, 2 * d:3 * d].repeat_interleave(N, dim=0)
    yf = y.float().cpu()
    yn = r16(r16(yf * torch.rsqrt(yf.pow(2).mean(-1, keepdim=True) + 1e-5)) * pw.float().cpu())
    xn = r16(x.float().cpu() + r16(gate * yn))
    assert rel_l2(xs, xn) < 2e-3
    if next_mode == 1:
        hn = r16(r16(xn * torch.rsqrt(xn.pow(2).mean(-1, keepdim=True) + 1e-5)) * nw.float().cpu())
        assert rel_l2(h, r16(hn * r16(1 + scale))) < 3e-3
    else:
        assert rel_l2(h, r16(torch.nn.functional.layer_norm(xn, (d,), None, None, 1e-6) * r16(1 + scale))) < 3e-3


# ---- the engine -------------------------------------------------------------------------------------------------------------------------

def test_imagenet_engine_matches_reference_golden_hd128(golden_dir):
    """Next-DiT-ImageNet DiT_Llama(dim=256, n_heads=2, n_layers=2) = head_dim 128 on a 16 x 16 latent (64 tokens: one whole key tile) against
    the unmodified reference, the bounds test_imagenet_engine_matches_reference_golden applies to imagenet_tiny"""
    g, cfg = _golden(golden_dir, "imagenet_tiny_hd128")
    assert cfg.head_dim == HD
    model = _build(models.imagenet.DiT_Llama, cfg, int(g["seed_w"]))
    z = torch.from_numpy(g["z"]).to("cuda", torch.bfloat16)
    t, y = torch.from_numpy(g["t"]).cuda(), torch.from_numpy(g["y"]).cuda()
    out = model(z, t, y)
    assert out.shape == z.shape and out.dtype == z.dtype
    assert rel_l2(out, torch.from_numpy(g["forward"])) < TOL_FWD, rel_l2(out, torch.from_numpy(g["forward"]))
    got = model.forward_with_cfg(z, t, y, 4.0)
    ref = torch.from_numpy(g["cfg4"])
    assert rel_l2(got, ref) < TOL_CFG4, rel_l2(got, ref)
    assert torch.equal(got[0, :3], got[1, :3]) and rel_l2(got[:, 3], ref[:, 3]) < TOL_FWD
    got = model.forward_with_cfg(z, t, y, 4.0, rope_scaling_factor=2.0, ntk_factor=1.5)
    assert rel_l2(got, torch.from_numpy(g["cfg4_rope"])) < TOL_CFG4
    model.forward_with_cfg(z, t, y, 1.0, rope_scaling_factor=1.0, ntk_factor=1.0)
    got = model.forward_with_cfg(z, t, y, 1.0)
    assert rel_l2(got, torch.from_numpy(g["cfg1_plain"])) < TOL_FWD
    # 5-point Euler trajectory through lt_sample_ode: finite, equal for the CFG halves on the guided channels, and at the reference's stored end point
    fn = Sampler(create_transport()).sample_ode(sampling_method="euler", num_steps=5)
    traj = fn(z, model.forward_with_cfg, y=y, cfg_scale=4.0)
    assert traj.shape == (5,) + tuple(z.shape) and torch.isfinite(traj.float()).all()
    assert torch.equal(traj[-1][0, :3], traj[-1][1, :3])  # guidance acts on channels [:3]: both rows carry the guided value
    assert rel_l2(traj[-1], torch.from_numpy(g["traj_euler"])[-1]) < TOL_CFG4


def test_full_imagenet_7b_32_layers_vs_reference(golden_dir):
    """DiT_Llama_7B_patch2(qk_norm=True), all 32 layers, dim 4096, head_dim 128, ffn 11008, 256 tokens, against the stored output of the
    unmodified reference module: the rule of tests/test_gpu_fulldepth.py::_check (engine <= 1.5 x min(floor, refbf16, refbf16ac), all
    channels and channel 3), then a 5-point Euler trajectory through lt_sample_ode on the same model"""
    _, model = FD._check("full_imagenet7b", golden_dir, lambda cfg: models.imagenet.DiT_Llama_7B_patch2(qk_norm=True, num_classes=cfg.num_classes),
                      keep=True)
    g, cfg = FD._load(golden_dir, "full_imagenet7b")
    z, t, y = FD._inputs(g, cfg, 0.5)
    zb = z.to("cuda", torch.bfloat16)
    fn = Sampler(create_transport()).sample_ode(sampling_method="euler", num_steps=5)
    traj = fn(zb, model.forward_with_cfg, y=y.cuda(), cfg_scale=4.0)
    assert traj.shape == (5,) + tuple(zb.shape) and torch.isfinite(traj.float()).all()
    assert torch.equal(traj[-1][0, :3], traj[-1][1, :3]) and not torch.equal(traj[-1], traj[0])


@pytest.mark.parametrize("family,ctor", [("moe", "DiT_Llama"), ("moe_time", "DiT_Llama_TimeMoE"), ("moe_space", "DiT_Llama_SpaceMoE")])
def test_moe_variants_run_at_head_dim_128(family, ctor):
    """the three MoE variants are no longer refused at head_dim 128: creation + one guided forward, finite and equal for the CFG halves"""
    cfg = synth.NextDiTConfig(dim=256, n_layers=2, n_heads=2, family=family, num_classes=10, num_experts=4 if family == "moe" else 8)
    model = _build(getattr(models.moe, ctor), cfg, 5)
    z, t, y = synth.synth_inputs(cfg, latent_hw=(16, 16), seed=6)
    got = model.forward_with_cfg(z.to("cuda", torch.bfloat16), t.cuda(), y.cuda(), 4.0)
    assert torch.isfinite(got.float()).all() and torch.equal(got[0, :3], got[1, :3]) and float(got.float().abs().max()) > 0


def test_text_variant_at_head_dim_128_is_refused_by_name():
    cfg = _lib.LtConfig(variant=_lib.LT_VARIANT_NEXT_T2I, dim=256, n_layers=1, n_heads=2, n_kv_heads=2, ffn_hidden=768, patch_size=2, in_channels=4,
                        out_channels=8, cap_feat_dim=128, adaln_dim=256, qk_norm=1, num_classes=0, norm_eps=1e-5, max_batch=2, max_tokens=64,
                        max_text=64, rope_table_len=384)
    handle = C.c_void_p()
    assert lib().lt_create(C.byref(cfg), C.byref(handle)) != 0
    assert b"head_dim 128 with text cross-attention not built" in lib().lt_last_error()
