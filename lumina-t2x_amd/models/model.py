"""Next-DiT (text-conditional) behind the reference's construction / checkpoint / call API.

Source compatibility target: ``lumina_next_t2i/models/model.py`` -
``models.__dict__[name](qk_norm=..., cap_feat_dim=...)`` (sample.py:125-128), ``.eval().to("cuda", dtype)``,
``load_state_dict(ckpt, strict=True)`` with the 567-key contract of SURVEY.md A.2, and
``forward(x, t, cap_feats, cap_mask)`` / ``forward_with_cfg(...)`` (model.py:836-913).

The module tree below only HOLDS parameters under the reference's key names; both call paths hand the
tensors to the HIP engine (``csrc/``) through the C ABI.  There is deliberately no PyTorch implementation of
the forward pass here: on a machine without the HIP extension or without a ROCm device the call raises.
"""
from __future__ import annotations

import functools
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib
from ..engine import DiTEngine, EngineLimits, _refuse_if_capturing, ffn_hidden_dim
from ._base import EngineSamplers, WeightWatch
from .components import AffineNorm, Linear, RMSNorm

_normal002 = functools.partial(nn.init.normal_, std=0.02)


class TimestepEmbedder(nn.Module):
    """keys: ``mlp.0.{weight,bias}``, ``mlp.2.{weight,bias}`` (reference model.py:37-60)."""

    def __init__(self, hidden_size: int, frequency_embedding_size: int = 256):
        super().__init__()
        self.mlp = nn.Sequential(
            Linear(frequency_embedding_size, hidden_size, bias=True, init=_normal002),
            nn.SiLU(),
            Linear(hidden_size, hidden_size, bias=True, init=_normal002),
        )
        self.frequency_embedding_size = frequency_embedding_size


class Attention(nn.Module):
    """keys: wq wk wv wo wk_y wv_y (no bias), gate, q_norm/k_norm/ky_norm (reference model.py:137-224)."""

    def __init__(self, dim: int, n_heads: int, n_kv_heads: Optional[int], qk_norm: bool, y_dim: int):
        super().__init__()
        self.n_heads = n_heads
        self.n_kv_heads = n_heads if n_kv_heads is None else n_kv_heads
        self.head_dim = dim // n_heads
        kv_dim = self.n_kv_heads * self.head_dim
        self.wq = Linear(dim, n_heads * self.head_dim, bias=False)
        self.wk = Linear(dim, kv_dim, bias=False)
        self.wv = Linear(dim, kv_dim, bias=False)
        if y_dim > 0:
            self.wk_y = Linear(y_dim, kv_dim, bias=False)
            self.wv_y = Linear(y_dim, kv_dim, bias=False)
            self.gate = nn.Parameter(torch.zeros([n_heads]))
        self.wo = Linear(n_heads * self.head_dim, dim, bias=False)
        if qk_norm:
            self.q_norm = AffineNorm(n_heads * self.head_dim)
            self.k_norm = AffineNorm(kv_dim)
            self.ky_norm = AffineNorm(kv_dim) if y_dim > 0 else nn.Identity()
        else:
            self.q_norm = self.k_norm = nn.Identity()
            self.ky_norm = nn.Identity()
        # kept for source compatibility: forward_with_cfg sets these per call (reference model.py:891-899)
        self.base_seqlen = None
        self.proportional_attn = False


class FeedForward(nn.Module):
    """keys: w1, w2, w3 (reference model.py:441-495)."""

    def __init__(self, dim: int, hidden_dim: int):
        super().__init__()
        self.w1 = Linear(dim, hidden_dim, bias=False)
        self.w2 = Linear(hidden_dim, dim, bias=False)
        self.w3 = Linear(dim, hidden_dim, bias=False)


class TransformerBlock(nn.Module):
    """Sandwich-norm block with tanh-gated adaLN (reference model.py:505-624)."""

    def __init__(self, layer_id: int, dim: int, n_heads: int, n_kv_heads: Optional[int], multiple_of: int,
                 ffn_dim_multiplier: Optional[float], norm_eps: float, qk_norm: bool, y_dim: int):
        super().__init__()
        self.dim = dim
        self.head_dim = dim // n_heads
        self.layer_id = layer_id
        self.attention = Attention(dim, n_heads, n_kv_heads, qk_norm, y_dim)
        self.feed_forward = FeedForward(dim, ffn_hidden_dim(dim, multiple_of, ffn_dim_multiplier))
        self.attention_norm1 = RMSNorm(dim, eps=norm_eps)
        self.ffn_norm1 = RMSNorm(dim, eps=norm_eps)
        self.attention_norm2 = RMSNorm(dim, eps=norm_eps)
        self.ffn_norm2 = RMSNorm(dim, eps=norm_eps)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), Linear(min(dim, 1024), 4 * dim, bias=True, init=nn.init.zeros_))
        self.attention_y_norm = RMSNorm(y_dim, eps=norm_eps)


class FinalLayer(nn.Module):
    """keys: ``linear.*``, ``adaLN_modulation.1.*`` (reference model.py:627-662; norm_final has no params)."""

    def __init__(self, hidden_size: int, patch_size: int, out_channels: int):
        super().__init__()
        self.linear = Linear(hidden_size, patch_size * patch_size * out_channels, bias=True, init=nn.init.zeros_)
        self.adaLN_modulation = nn.Sequential(
            nn.SiLU(), Linear(min(hidden_size, 1024), hidden_size, bias=True, init=nn.init.zeros_))


class CapEmbedder(nn.Sequential):
    pass


class NextDiT(EngineSamplers, WeightWatch, nn.Module):
    """Diffusion transformer whose forward passes execute on the MI355X engine.

    Constructor signature and defaults follow the reference (model.py:670-685).  Extra, engine-only knobs
    are keyword-only attributes set after construction: ``engine_limits`` (workspace sizing).
    """

    def __init__(self, patch_size: int = 2, in_channels: int = 4, dim: int = 4096, n_layers: int = 32,
                 n_heads: int = 32, n_kv_heads: Optional[int] = None, multiple_of: int = 256,
                 ffn_dim_multiplier: Optional[float] = None, norm_eps: float = 1e-5, learn_sigma: bool = True,
                 qk_norm: bool = False, cap_feat_dim: int = 5120, scale_factor: float = 1.0,
                 use_flash_attn: bool = True) -> None:
        # use_flash_attn: constructor kwarg of the mini package (lumina_next_t2i_mini/models/nextdit.py:637; sample.py:111) -
        # accepted so its scripts swap in unchanged; the engine has one attention path (exact softmax either way)
        super().__init__()
        self.use_flash_attn = use_flash_attn
        assert (dim // n_heads) % 4 == 0, "2d rope needs head dim to be divisible by 4"
        self.learn_sigma = learn_sigma
        self.in_channels = in_channels
        self.out_channels = in_channels * 2 if learn_sigma else in_channels
        self.patch_size = patch_size
        self.dim, self.n_heads, self.n_layers = dim, n_heads, n_layers
        self.n_kv_heads = n_heads if n_kv_heads is None else n_kv_heads
        self.norm_eps, self.qk_norm, self.cap_feat_dim = norm_eps, qk_norm, cap_feat_dim
        self.scale_factor = scale_factor
        self.ffn_hidden = ffn_hidden_dim(dim, multiple_of, ffn_dim_multiplier)

        self.x_embedder = Linear(patch_size * patch_size * in_channels, dim, bias=True)
        self.t_embedder = TimestepEmbedder(min(dim, 1024))
        cap_ln = AffineNorm(cap_feat_dim)
        self.cap_embedder = CapEmbedder(cap_ln, Linear(cap_feat_dim, min(dim, 1024), bias=True, init=nn.init.zeros_))
        self.layers = nn.ModuleList([
            TransformerBlock(i, dim, n_heads, n_kv_heads, multiple_of, ffn_dim_multiplier, norm_eps, qk_norm, cap_feat_dim)
            for i in range(n_layers)
        ])
        self.final_layer = FinalLayer(dim, patch_size, self.out_channels)
        self.pad_token = nn.Parameter(torch.empty(dim))
        nn.init.normal_(self.pad_token, std=0.02)

        self.engine_limits = EngineLimits()
        self._engine: Optional[DiTEngine] = None
        self._weights_sig = None

    # ---- engine plumbing (the weight-change check is WeightWatch._signature, models/_base.py) -------------------------
    def engine(self, x: torch.Tensor, text_len: int) -> DiTEngine:
        """Create / resize the engine for this call's shapes and make sure it holds the current weights."""
        if not (x if isinstance(x, torch.Tensor) else x[0]).is_cuda:
            raise _lib.LuminaLibError(
                "NextDiT.forward needs tensors on a ROCm device: the MI355X engine has no CPU fallback")
        if isinstance(x, torch.Tensor):
            B, _, H, W = x.shape
            n_tok = (H // self.patch_size) * (W // self.patch_size)
        else:  # list of [C, H_b, W_b] samples: limits of the padded batch
            B = len(x)
            n_tok = max((xi.shape[1] // self.patch_size) * (xi.shape[2] // self.patch_size) for xi in x)
            x = x[0]
        lim = self.engine_limits
        need = EngineLimits(max(lim.max_batch, B), max(lim.max_tokens, n_tok), max(lim.max_text, text_len))
        if self._engine is None or need != self._engine.limits or self._engine.device != x.device:
            # (before the old engine is dropped: its buffers may be what a graph the caller recorded earlier reads)
            _refuse_if_capturing(f"{type(self).__name__}: a new engine for this call's shapes (lt_create)")
            self._engine = None
            self._engine = DiTEngine(
                variant=_lib.LT_VARIANT_NEXT_T2I, dim=self.dim, n_layers=self.n_layers, n_heads=self.n_heads,
                n_kv_heads=self.n_kv_heads, ffn_hidden=self.ffn_hidden, patch_size=self.patch_size,
                in_channels=self.in_channels, out_channels=self.out_channels, cap_feat_dim=self.cap_feat_dim,
                qk_norm=self.qk_norm, norm_eps=self.norm_eps, limits=need, device=x.device)
            self.engine_limits = need
            self._weights_sig = None
        sig = self._signature()
        if sig != self._weights_sig:
            self._engine.load_state_dict(self.state_dict())
            self._weights_sig = sig
        return self._engine

    def _call(self, x, t, cap_feats, cap_mask, use_cfg, **kw):
        eng = self.engine(x, cap_feats.shape[1])
        eng.prepare_prompt(cap_feats, cap_mask)
        if not isinstance(x, torch.Tensor):  # variable-resolution packing (model.py:789-834): plain forward only, like the reference
            if use_cfg:
                raise TypeError("forward_with_cfg takes a [B, C, H, W] tensor (reference model.py:901-902)")
            if len(kw.pop("skip_layers", ())):
                raise _lib.LuminaLibError("forward: skip_layers on a packed batch (a list of latents) is not served")
            if len(kw.pop("perturb_layers", ())):
                raise _lib.LuminaLibError("forward: perturb_layers on a packed batch (a list of latents) is not served")
            if len(kw.pop("blur_layers", ())):
                raise _lib.LuminaLibError("forward: blur_layers on a packed batch (a list of latents) is not served")
            kw.pop("blur_sigma", None)
            return eng.forward_packed(list(x), t, **kw)
        return eng.forward(x, t, use_cfg=use_cfg, **kw)

    # ---- reference call surface ---------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x, t, cap_feats, cap_mask, skip_layers=(), perturb_layers=(), blur_layers=(), blur_sigma=None):
        """reference model.py:836-864; ``x`` is a [B, C, H, W] tensor or a list of [C, H_b, W_b] tensors of different sizes
        (returns a list then).  ``skip_layers`` (not in the reference; tensor input): the blocks left out of this evaluation, which are then
        the identity on the residual stream (lt_forward_skip); ``perturb_layers`` (likewise): the blocks whose self-attention map is
        replaced by the identity, the text cross-attention kept (lt_forward_perturb); ``blur_layers`` with ``blur_sigma`` (likewise): the blocks whose self-attention reads
        queries blurred over the token grid (lt_forward_blur); all empty: the call it was"""
        return self._call(x, t, cap_feats, cap_mask, False, skip_layers=tuple(skip_layers), perturb_layers=tuple(perturb_layers),
                          blur_layers=tuple(blur_layers), blur_sigma=blur_sigma,
                          **self._plain_forward_args())

    def _plain_forward_args(self) -> dict:
        """what the reference's plain ``forward`` reads off the module (model.py:836-864): the attention flags left on the
        layers by the last forward_with_cfg (:891-899), and the RoPE table left in self.freqs_cis - after construction
        that is the NTK branch at the constructor's scale_factor (:732-736) -> watershed 0 selects it for any t.  (The
        reference also re-uses a table rebuilt by a forward_with_cfg with OTHER scaling arguments; the engine keeps the
        constructor's - documented difference, the reference's samplers never mix the two on one module.)"""
        pa = self.layers[0].attention.proportional_attn if self.n_layers else False
        bs = self.layers[0].attention.base_seqlen if self.n_layers else None
        return dict(scale_factor=self.scale_factor, scale_watershed=0.0, proportional_attn=pa, base_seqlen=bs)

    @torch.no_grad()
    def forward_with_cfg(self, x, t, cap_feats, cap_mask, cfg_scale, scale_factor=1.0, scale_watershed=1.0,
                         base_seqlen: Optional[int] = None, proportional_attn: bool = False):
        """reference model.py:866-913: batch = cat([half, half]); CFG on channels [:3] only."""
        if proportional_attn:
            assert base_seqlen is not None
        for layer in self.layers:  # mirrored attributes (reference model.py:891-899)
            layer.attention.base_seqlen = base_seqlen if proportional_attn else None
            layer.attention.proportional_attn = proportional_attn
        return self._call(x, t, cap_feats, cap_mask, True, cfg_scale=cfg_scale, scale_factor=scale_factor,
                          scale_watershed=scale_watershed, base_seqlen=base_seqlen, proportional_attn=proportional_attn)

    def _packed_cfg_engine(self, xs, cap_feats, cap_mask, base_seqlen, proportional_attn):
        xs = list(xs)
        if len(xs) != cap_feats.shape[0]:
            raise _lib.LuminaLibError(f"packed guidance: {len(xs)} samples (cond rows, then uncond rows) need as many prompt rows, got "
                                      f"{cap_feats.shape[0]}")
        if proportional_attn:
            assert base_seqlen is not None
        for layer in self.layers:  # mirrored attributes (reference model.py:891-899)
            layer.attention.base_seqlen = base_seqlen if proportional_attn else None
            layer.attention.proportional_attn = proportional_attn
        eng = self.engine(xs, cap_feats.shape[1])
        eng.prepare_prompt(cap_feats, cap_mask)
        return eng, xs

    @torch.no_grad()
    def forward_with_cfg_packed(self, xs, t, cap_feats, cap_mask, cfg_scale, scale_factor=1.0, scale_watershed=1.0,
                                base_seqlen: Optional[int] = None, proportional_attn: bool = False):
        """forward_with_cfg on a LIST of 2 B' latents ``[C, H_b, W_b]`` (cond rows, then uncond rows of the same sizes): the reference's list
        ``forward`` (model.py:789-834) on ``[x_0 .. x_{B'-1}] * 2`` and the guidance expression of :901-913 per sample.  Returns a list."""
        eng, xs = self._packed_cfg_engine(xs, cap_feats, cap_mask, base_seqlen, proportional_attn)
        return eng.forward_cfg_packed(xs, t, cfg_scale=cfg_scale, scale_factor=scale_factor, scale_watershed=scale_watershed,
                                      base_seqlen=base_seqlen, proportional_attn=proportional_attn)

    @torch.no_grad()
    def sample_ode_packed(self, zs, tgrid, cap_feats, cap_mask, cfg_scale, method: str = "midpoint", return_trajectory: bool = False,
                          scale_factor=1.0, scale_watershed=1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False):
        """the fixed-grid ODE trajectory of a LIST of differently sized latents in ONE engine call, every evaluation
        ``forward_with_cfg_packed``.  ``method``: euler / midpoint / rk4 (lt_sample_ode_packed) or a multistep method ab2 / ab3 / abm2 / abm3
        (lt_sample_ode_multistep_packed).  Returns one tensor per sample: the last state, or ``[len(tgrid), C, H_b, W_b]``."""
        eng, zs = self._packed_cfg_engine(zs, cap_feats, cap_mask, base_seqlen, proportional_attn)
        if method in _lib.ODE_MULTISTEP_METHODS:
            return eng.sample_ode_multistep_packed(zs, tgrid, method, use_cfg=True, cfg_scale=cfg_scale, scale_factor=scale_factor,
                                                   scale_watershed=scale_watershed, base_seqlen=base_seqlen, proportional_attn=proportional_attn,
                                                   return_trajectory=return_trajectory)
        return eng.sample_ode_packed(zs, tgrid, method, use_cfg=True, cfg_scale=cfg_scale, scale_factor=scale_factor,
                                     scale_watershed=scale_watershed, base_seqlen=base_seqlen, proportional_attn=proportional_attn,
                                     return_trajectory=return_trajectory)

    @torch.no_grad()
    def sample_ode_masked(self, z, tgrid, mask, x1, noise, cap_feats, cap_mask, cfg_scale, method: str = "midpoint",
                          return_trajectory: bool = False, scale_factor=1.0, scale_watershed=1.0, base_seqlen: Optional[int] = None,
                          proportional_attn: bool = False):
        """Inpainting in ONE engine call (lt_sample_ode_masked): the fixed-grid trajectory of ``z [B, C, H, W]`` over ``tgrid`` with
        ``y = y * mask + (noise * (1 - t) + x1 * t) * (1 - mask)`` after every full step.  ``mask`` (1 = generate, 0 = keep; ``[H, W]`` or
        ``[1|B, 1, H, W]``), the source latent ``x1`` and the ``noise`` the trajectory started from (``[1|B', C, H, W]``) are broadcast to the
        state and repeated for the uncond half (``transport.masked.expand_operands``).  Every evaluation is ``forward_with_cfg``; with
        ``cfg_scale=None`` it is the plain ``forward``.  Returns the last state, or all ``len(tgrid)`` states."""
        from ..transport.masked import expand_operands
        use_cfg = cfg_scale is not None
        kw = dict(cap_feats=cap_feats, cap_mask=cap_mask)
        if use_cfg:
            if proportional_attn:
                assert base_seqlen is not None
            for layer in self.layers:  # mirrored attributes (reference model.py:891-899)
                layer.attention.base_seqlen = base_seqlen if proportional_attn else None
                layer.attention.proportional_attn = proportional_attn
            kw.update(cfg_scale=cfg_scale, scale_factor=scale_factor, scale_watershed=scale_watershed, base_seqlen=base_seqlen,
                      proportional_attn=proportional_attn)
        m, src, nz = expand_operands(z, mask, x1, noise)
        eng, args = self._engine_sampler_args(z, use_cfg, kw)
        return eng.sample_ode_masked(z, tgrid, m, src, nz, method, use_cfg=use_cfg, return_trajectory=return_trajectory, **args)

    @torch.no_grad()
    def sample_ode_masked_packed(self, zs, tgrid, masks, x1s, noises, cap_feats, cap_mask, cfg_scale, method: str = "midpoint",
                                 return_trajectory: bool = False, scale_factor=1.0, scale_watershed=1.0, base_seqlen: Optional[int] = None,
                                 proportional_attn: bool = False):
        """``sample_ode_masked`` on a LIST of differently sized latents (lt_sample_ode_masked_packed), every evaluation
        ``forward_with_cfg_packed``: ``masks`` / ``x1s`` / ``noises`` are lists with one entry per sample, or one per sample of the cond half
        (repeated for the uncond half), each broadcasting to its sample ``[C, H_b, W_b]``.  Returns one tensor per sample."""
        from ..transport.masked import expand_operands_packed
        zs = list(zs)
        ms, srcs, nzs = expand_operands_packed(zs, masks, x1s, noises)
        eng, zs = self._packed_cfg_engine(zs, cap_feats, cap_mask, base_seqlen, proportional_attn)
        return eng.sample_ode_masked_packed(zs, tgrid, ms, srcs, nzs, method, use_cfg=True, cfg_scale=cfg_scale, scale_factor=scale_factor,
                                            scale_watershed=scale_watershed, base_seqlen=base_seqlen, proportional_attn=proportional_attn,
                                            return_trajectory=return_trajectory)

    def _engine_sampler_args(self, x, use_cfg, kw):
        """transport fast paths (models/_base.py: EngineSamplers): kwargs of forward_with_cfg / forward -> engine + step kwargs"""
        cap_feats, cap_mask = kw.pop("cap_feats"), kw.pop("cap_mask")
        if use_cfg:
            args = dict(cfg_scale=kw.pop("cfg_scale"), scale_factor=kw.pop("scale_factor", 1.0),
                        scale_watershed=kw.pop("scale_watershed", 1.0), base_seqlen=kw.pop("base_seqlen", None),
                        proportional_attn=kw.pop("proportional_attn", False))
        else:
            args = self._plain_forward_args()  # the same module state a per-step forward() would read
        if kw:
            raise TypeError(f"unexpected model kwargs for the engine path: {sorted(kw)}")
        eng = self.engine(x, cap_feats.shape[1])
        eng.prepare_prompt(cap_feats, cap_mask)
        return eng, args

    @torch.no_grad()
    def sample_views(self, z, tgrid, views, cap_feats, cap_mask, method: str = "midpoint", *, cfg_scale: float = 4.0,
                     return_trajectory: bool = True):
        """Multi-view (visual-anagram) sampling, Phase Init of the reference's visual_anagrams/generate.py:389-414, on the engine: ONE latent
        ``z [1, C, H, W]``, V ``views`` (``lumina_t2x_amd.views``), ``cap_feats [2V, T, D]`` / ``cap_mask [2V, T]`` with rows 0..V-1 the view
        prompts and rows V..2V-1 the negative prompt.  Every stage of every interval is one forward_with_cfg of 2 V rows.  Phase Init
        passes ``cfg_scale`` only (scale_factor 1, no proportional attention); Phase Upscale is ``sample_views_guided``."""
        V = len(views)
        if cap_feats.shape[0] != 2 * V:
            raise _lib.LuminaLibError(f"sample_views: {V} views need 2 V = {2 * V} prompt rows (view prompts, then the negative prompt per "
                                      f"view), got {cap_feats.shape[0]}")
        for layer in self.layers:  # what a forward_with_cfg without proportional attention leaves on the module
            layer.attention.base_seqlen = None
            layer.attention.proportional_attn = False
        eng = self.engine(z.expand(2 * V, -1, -1, -1), cap_feats.shape[1])
        eng.prepare_prompt(cap_feats, cap_mask)
        eng.set_views(views, z.shape[2], z.shape[3])
        return eng.sample_views(z, tgrid, method, cfg_scale=cfg_scale, return_trajectory=return_trajectory)

    @torch.no_grad()
    def sample_views_guided(self, z, guidance, tgrid, views, cap_feats, cap_mask, *, noise=None, cfg_scale: float = 4.0,
                            scale_factor: float = 1.0, scale_watershed=None, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                            coef_rounding: str = "fp32", return_trajectory: bool = True):
        """Phase Upscale of the reference's visual_anagrams/generate.py:465-494 on the engine, all V views of a stage in one forward_with_cfg of
        2 V rows and the whole phase in ONE call: the stepping rule is ``midpoint_solver_extra`` (:222-262), whose model input blends the state
        with the ``guidance`` latent and the initial ``noise`` (default: ``z``).  Prompt layout as ``sample_views``.  The model is the anagram
        fork's (visual_anagrams/models/nextdit.py): its softmax rule and its ``ntk_v1`` RoPE (``scale_watershed = 0``) are set for this call and
        restored afterwards; a caller's ``scale_watershed`` is ignored, as the fork ignores it.  ``coef_rounding``: ``"fp32"`` (default) keeps
        the decay factor ``c`` in fp32 when it multiplies the state - the expected behaviour of the reference's GPU run, not verified on one;
        ``"state"`` rounds it to the state dtype first, which is what the reference's CPU bf16 run does (``views_guided_table``)."""
        from ..transport.integrators import views_guided_table
        V = len(views)
        if cap_feats.shape[0] != 2 * V:
            raise _lib.LuminaLibError(f"sample_views_guided: {V} views need 2 V = {2 * V} prompt rows (view prompts, then the negative prompt per "
                                      f"view), got {cap_feats.shape[0]}")
        if proportional_attn:
            assert base_seqlen is not None
        for layer in self.layers:  # mirrored attributes (nextdit.py:889-897)
            layer.attention.base_seqlen = base_seqlen if proportional_attn else None
            layer.attention.proportional_attn = proportional_attn
        coef = views_guided_table(tgrid, z.dtype, coef_rounding)
        eng = self.engine(z.expand(2 * V, -1, -1, -1), cap_feats.shape[1])
        eng.prepare_prompt(cap_feats, cap_mask)
        eng.set_views(views, z.shape[2], z.shape[3])
        before = getattr(eng, "softmax_rule", _lib.LT_SOFTMAX_T2I)
        eng.set_softmax_rule(_lib.LT_SOFTMAX_ANAGRAM)
        try:
            return eng.sample_views_guided(z, guidance, tgrid, coef, noise=noise, cfg_scale=cfg_scale, scale_factor=scale_factor,
                                           scale_watershed=0.0, base_seqlen=base_seqlen, proportional_attn=proportional_attn,
                                           return_trajectory=return_trajectory)
        finally:
            eng.set_softmax_rule(before)

    def parameter_count(self) -> int:
        return sum(p.numel() for p in self.parameters())

    def get_fsdp_wrap_module_list(self):
        return list(self.layers)

    def get_checkpointing_wrap_module_list(self):
        return list(self.layers)


def NextDiT_2B_patch2(**kwargs):
    """reference model.py:994-995"""
    return NextDiT(patch_size=2, dim=2304, n_layers=24, n_heads=32, **kwargs)


def NextDiT_2B_GQA_patch2(**kwargs):
    """reference model.py:998-999"""
    return NextDiT(patch_size=2, dim=2304, n_layers=24, n_heads=32, n_kv_heads=8, **kwargs)
