"""Thin PyTorch-side plumbing around the C-ABI engine: tensors in, tensors out, current HIP stream.

PyTorch only supplies device memory, streams and (elsewhere) ``torch.distributed``; every FLOP of the
denoising path runs in the HIP kernels behind ``liblumina_dit.so``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import _lib
from ._lib import LtConfig, LtStepArgs, LuminaLibError

_DT = {torch.float32: _lib.LT_F32, torch.bfloat16: _lib.LT_BF16, torch.float16: _lib.LT_F16}
_STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}  # model evaluations per interval of the fixed-grid methods


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _refuse_if_capturing(who: str) -> None:
    """the calls that create an engine or upload weights allocate and synchronise: inside the caller's ``torch.cuda.graph`` they would end
    the capture with an error, so they are refused by name before they touch the device"""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise LuminaLibError(f"{who}: refused on a stream under capture: it allocates and synchronises, which a graph cannot record - run one "
                             "eager evaluation of this shape before the capture begins")


def _require_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise LuminaLibError(
            f"{name} lives on {t.device}; the MI355X denoising engine only runs on a ROCm device "
            "(there is no CPU fallback - use oracle/ for CPU reference numbers in tests)"
        )


def _refusing(check, *args, who: Optional[str] = None, **kw):
    """the result of a host-side check of the transport package (``check_*`` / ``refuse_*``: they raise ``ValueError``); what it objects to is
    the engine's refusal, a ``LuminaLibError`` of the same words behind an optional ``"{who}: "``"""
    try:
        return check(*args, **kw)
    except ValueError as exc:
        raise LuminaLibError(f"{who}: {exc}" if who else str(exc)) from None


def _grid_array(tgrid):
    """a fixed time grid (tensor or sequence) as a C float array of its fp32 values, and its length"""
    t = tgrid if isinstance(tgrid, torch.Tensor) else torch.tensor(list(tgrid), dtype=torch.float32)
    grid = [float(v) for v in t.detach().to("cpu", torch.float32).tolist()]
    return (C.c_float * len(grid))(*grid), len(grid)


def _traj_or_final(z: torch.Tensor, n: int, state_shape, return_trajectory: bool):
    """the output buffer of a whole-trajectory call and its (trajectory, final) pointers: all ``n`` states ``[n, *state_shape]`` or the
    last one alone, shaped like ``z`` - the other pointer is null"""
    out = torch.empty((n,) + tuple(state_shape), dtype=z.dtype, device=z.device) if return_trajectory else torch.empty_like(z)
    ptr, null = C.c_void_p(out.data_ptr()), C.c_void_p(0)
    return (out, ptr, null) if return_trajectory else (out, null, ptr)


class _SourceCache:
    """Remembers WHICH tensors the engine's conditioning was prepared from, so that the per-step calls of an ODE solve (same
    ``model_kwargs`` objects every step) do not redo the caption work.  A hit needs the very same tensor objects, unmodified
    (``_version``); the cache keeps them referenced, so their storage cannot be freed and handed to a different prompt that
    would then look identical by address."""

    def __init__(self):
        self._src = None
        self._key = None

    @staticmethod
    def _describe(tensors, extra):
        return (tuple((t._version, tuple(t.shape), t.dtype, t.device) for t in tensors), tuple(extra))

    @staticmethod
    def _trackable(tensors) -> bool:
        # inference tensors (torch.inference_mode) carry no version counter: in-place edits cannot be seen, so never cache them
        return not any(t.is_inference() for t in tensors)

    def hit(self, tensors, extra=()) -> bool:
        # one read of each field: set_option() on another thread may clear() between two of them (a miss then, never a TypeError)
        src, key = self._src, self._key
        return (src is not None and self._trackable(tensors) and len(src) == len(tensors)
                and all(a is b for a, b in zip(src, tensors)) and key == self._describe(tensors, extra))

    def store(self, tensors, extra=()) -> None:
        if not self._trackable(tensors):
            self.clear()
            return
        self._src, self._key = tuple(tensors), self._describe(tensors, extra)

    def clear(self) -> None:
        self._src = self._key = None


@dataclass
class EngineLimits:
    max_batch: int = 2
    max_tokens: int = 4096
    max_text: int = 256


class DiTEngine:
    """Owns one ``lt_engine`` handle (weights arena + workspace in HBM) for one model on one GPU."""

    def __init__(self, *, variant: int, dim: int, n_layers: int, n_heads: int, n_kv_heads: int, ffn_hidden: int,
                 patch_size: int, in_channels: int, out_channels: int, cap_feat_dim: int, qk_norm: bool,
                 norm_eps: float, num_classes: int = 0, num_experts: int = 0, limits: Optional[EngineLimits] = None,
                 device: Optional[torch.device] = None):
        _refuse_if_capturing("DiTEngine (lt_create)")
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda")
        if not torch.cuda.is_available():
            raise LuminaLibError("no ROCm device visible: the denoising engine cannot run (no CPU fallback)")
        lim = limits or EngineLimits()
        self.limits = lim
        cfg = LtConfig(
            variant=variant, dim=dim, n_layers=n_layers, n_heads=n_heads, n_kv_heads=n_kv_heads,
            ffn_hidden=ffn_hidden, patch_size=patch_size, in_channels=in_channels, out_channels=out_channels,
            cap_feat_dim=cap_feat_dim, adaln_dim=min(dim, 1024), qk_norm=int(bool(qk_norm)), num_classes=num_classes,
            norm_eps=norm_eps, max_batch=lim.max_batch, max_tokens=lim.max_tokens, max_text=lim.max_text,
            rope_table_len=384, num_experts=num_experts,
        )
        self.cfg = cfg
        self.in_channels = in_channels
        self.patch_size = patch_size
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.lt_create(C.byref(cfg), C.byref(handle)), "lt_create")
        self.handle = handle
        self._prompt = _SourceCache()
        self.num_classes = num_classes

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                self.lib.lt_destroy(h)
            except Exception:
                pass
            self.handle = None

    # ---- the binding: the one way into the library, and what a call is given ------------------------
    def _call(self, name: str, *args) -> None:
        """``name(handle, *args)`` on this engine's device; a non-zero status is raised under the entry's own name"""
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(self.handle, *args)
        _lib.check(rc, name)

    def _stream(self) -> C.c_void_p:
        """the caller's current stream on this engine's device, for the place the entry's signature gives the stream"""
        return C.c_void_p(_stream_ptr(self.device))

    @staticmethod
    def _dev(t: Optional[torch.Tensor]) -> C.c_void_p:
        """a device tensor's address; null for ``None``.  (The callers keep the tensor: it is their argument, their result or ``_keep``.)"""
        return C.c_void_p(t.data_ptr() if t is not None else 0)

    @staticmethod
    def _host(t: Optional[torch.Tensor]):
        """a contiguous fp32 / int32 CPU tensor as the ``float *`` / ``int32_t *`` the entry reads during the call; ``None`` (null) for
        ``None``.  The pointer object holds the tensor (``_tensor``) and the call's argument list holds the pointer object, so the memory
        stays allocated until the call returns, also when the tensor was a temporary of the caller's expression."""
        if t is None:
            return None
        ptr = C.cast(t.data_ptr(), C.POINTER(C.c_int32 if t.dtype == torch.int32 else C.c_float))
        ptr._tensor = t
        return ptr

    @staticmethod
    def _table(values, count: Optional[int] = None, wrong=None, dtype=torch.float32) -> torch.Tensor:
        """a host table (a tensor or a sequence) as a flat contiguous CPU tensor of ``dtype``; ``count``: the entries it must have, and
        ``wrong(entries)`` the words of the refusal when it has another number (its contents are the C entry's to check).  A sequence is
        read as fp32 numbers, whatever ``dtype``: a table of another type (the int32 reuse flags) comes in as a tensor."""
        tab = values if isinstance(values, torch.Tensor) else torch.tensor(list(values), dtype=torch.float32)
        tab = tab.detach().to("cpu", dtype).reshape(-1).contiguous()
        if count is not None and tab.numel() != count:
            raise LuminaLibError(wrong(tab.numel()))
        return tab

    @staticmethod
    def _eval_io(x: torch.Tensor, t: torch.Tensor, *, out: Optional[torch.Tensor] = None, writes: bool = True, name: str = "x"):
        """the operands of one evaluation: ``(x contiguous, t in fp32 on x's device, the tensor to write)`` - the caller's ``out``, else a
        new one like ``x``, or none for an evaluation that writes no tensor (``writes=False``); ``name``: what a refusal calls ``x``"""
        _require_gpu(x, name)
        x = x.contiguous()
        t32 = t.to(device=x.device, dtype=torch.float32).contiguous()
        if out is None and writes:
            out = torch.empty_like(x)
        return x, t32, out

    @staticmethod
    def _fixed_grid(method: str, tgrid, refusal: Optional[str] = None):
        """a fixed-grid trajectory's ``(grid array, grid points n, method code, model evaluations)``; ``refusal``: the entry's own words
        for a method that is not euler / midpoint / rk4"""
        if method not in _lib.ODE_METHODS:
            raise LuminaLibError(refusal or f"fixed-grid method '{method}' not in {sorted(_lib.ODE_METHODS)}")
        garr, n = _grid_array(tgrid)
        return garr, n, _lib.ODE_METHODS[method], max(n - 1, 0) * _STAGES[method]

    def _stage_table(self, table, who: str, n: int, method: str, count: int) -> torch.Tensor:
        """the guidance scale of every stage of a fixed-grid trajectory"""
        return self._table(table, count, lambda got: f"{who}: the table has {got} entries, a {n}-point {method} grid has {count} stages")

    @staticmethod
    def _unpacked(out: torch.Tensor, spans, n: Optional[int] = None):
        """a packed result as one tensor per sample, views of the one allocation: ``[n, *shape]`` of the trajectory ``out [n, total]``, or
        (``n=None``) ``shape`` of the flat ``out``"""
        if n is not None:
            return [out[:, off:off + math.prod(shape)].view((n,) + shape) for off, shape in spans]
        return [out[off:off + math.prod(shape)].view(shape) for off, shape in spans]

    # ---- options (include/lumina_dit_debug.h) ----------------------------------------------------------
    def set_option(self, name: str, value: Optional[int]) -> None:
        """override one kernel-selection option for THIS engine only (``None`` drops the override: the process default set by
        ``lt_set_option`` applies again)"""
        v = _lib.LT_OPTION_INHERIT if value is None else int(value)
        _lib.check(self.lib.lt_engine_set_option(self.handle, name.encode(), v), f"lt_engine_set_option({name})")
        self._prompt.clear()  # the hoisted text K / V may depend on the option (rmsnorm_apex): prepare the conditioning again

    def get_option(self, name: str) -> int:
        """the value in effect for this engine (its override, else the process default)"""
        out = C.c_int32(0)
        _lib.check(self.lib.lt_engine_get_option(self.handle, name.encode(), C.byref(out)), f"lt_engine_get_option({name})")
        return int(out.value)

    # ---- weights ---------------------------------------------------------------------------------
    def load_state_dict(self, state: Dict[str, torch.Tensor], skip: Iterable[str] = ()) -> None:
        """Upload every tensor of a reference-format state_dict into the engine."""
        # the hoisted conditioning (text K / V of every layer, caption / label embedding) was computed from the OLD weights:
        # forget which tensors it came from, so the next call prepares it again (lt_set_weight also invalidates it engine-side)
        _refuse_if_capturing("load_state_dict (lt_set_weight)")
        self._prompt.clear()
        s = self._stream()
        skip = set(skip)
        with torch.cuda.device(self.device):
            for key, t in state.items():
                if key in skip:
                    continue
                t = t.detach()
                if t.device != self.device or t.dtype not in _DT or not t.is_contiguous():
                    dt = t.dtype if t.dtype in _DT else torch.float32
                    t = t.to(device=self.device, dtype=dt).contiguous()
                shape = (C.c_int64 * max(t.dim(), 1))(*(t.shape if t.dim() else (1,)))
                rc = self.lib.lt_set_weight(self.handle, key.encode(), self._dev(t), _DT[t.dtype], shape, max(t.dim(), 1), s)
                _lib.check(rc, f"lt_set_weight({key})")
            torch.cuda.current_stream(self.device).synchronize()  # sources may be temporaries
            self._call("lt_weights_ready")

    # ---- prompt ----------------------------------------------------------------------------------
    def prepare_prompt(self, cap_feats: torch.Tensor, cap_mask: torch.Tensor) -> None:
        _require_gpu(cap_feats, "cap_feats")
        if self._prompt.hit((cap_feats, cap_mask), ("prompt",)):
            return
        feats = cap_feats if cap_feats.dtype in (torch.float32, torch.bfloat16) else cap_feats.float()
        feats = feats.contiguous()
        mask = cap_mask.to(device=feats.device, dtype=torch.int32).contiguous()
        B, T, _ = feats.shape
        self._call("lt_prepare_prompt", self._dev(feats), _DT[feats.dtype], self._dev(mask), B, T, self._stream())
        self._keep = (feats, mask)  # keep the temporaries alive until the stream has consumed them
        self._prompt.store((cap_feats, cap_mask), ("prompt",))

    def prepare_prompt_regional(self, cap_feats: torch.Tensor, cap_mask: torch.Tensor, global_feats: torch.Tensor,
                                global_mask: torch.Tensor, h_split: int, w_split: int) -> None:
        """compositional Next-DiT: Y captions (regions of the cond row ..., uncond row) + the one-row global caption"""
        _require_gpu(cap_feats, "cap_feats")
        src, extra = (cap_feats, cap_mask, global_feats, global_mask), ("regional", int(h_split), int(w_split))
        if self._prompt.hit(src, extra):
            return
        dt = cap_feats.dtype if cap_feats.dtype in (torch.float32, torch.bfloat16) else torch.float32
        feats = cap_feats.to(dt).contiguous()
        gfeats = global_feats.to(device=feats.device, dtype=dt).contiguous()
        mask = cap_mask.to(device=feats.device, dtype=torch.int32).contiguous()
        gmask = global_mask.to(device=feats.device, dtype=torch.int32).contiguous()
        Y, T, _ = feats.shape
        self._call("lt_prepare_prompt_regional", self._dev(feats), _DT[feats.dtype], self._dev(mask), Y, T, self._dev(gfeats),
                   self._dev(gmask), gfeats.shape[1], int(h_split), int(w_split), self._stream())
        self._keep = (feats, mask, gfeats, gmask)
        self._prompt.store(src, extra)

    def prepare_labels(self, y: torch.Tensor) -> None:
        """class-conditional variants: y int [B] (null class = num_classes, Next-DiT-ImageNet/sample.py:181)"""
        _require_gpu(y, "y")
        if self._prompt.hit((y,), ("labels",)):
            return
        lab = y.to(dtype=torch.int32).contiguous()
        self._call("lt_prepare_labels", self._dev(lab), lab.numel(), self._stream())
        self._keep = (lab,)
        self._prompt.store((y,), ("labels",))

    # ---- one model evaluation --------------------------------------------------------------------
    def _step_args(self, x: torch.Tensor, cfg_scale: float, scale_factor: float, scale_watershed: float,
                   base_seqlen: Optional[int], proportional_attn: bool, cfg_channels: int = 3,
                   ntk_factor: float = 1.0) -> LtStepArgs:
        B, Cc, H, W = x.shape
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise LuminaLibError(f"state dtype {x.dtype} unsupported (bf16 or fp32)")
        return LtStepArgs(cfg_scale=float(cfg_scale), scale_factor=float(scale_factor),
                          scale_watershed=float(scale_watershed), base_seqlen=int(base_seqlen or 0),
                          proportional_attn=int(bool(proportional_attn)), latent_h=H, latent_w=W, batch=B,
                          io_dtype=_DT[x.dtype], cfg_channels=cfg_channels, ntk_factor=float(ntk_factor))

    def forward(self, x: torch.Tensor, t: torch.Tensor, *, use_cfg: bool, cfg_scale: float = 1.0,
                scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                proportional_attn: bool = False, ntk_factor: float = 1.0, skip_layers=(), perturb_layers=(), blur_layers=(),
                blur_sigma=None) -> torch.Tensor:
        """one evaluation; ``skip_layers`` (plain forward only): the blocks left out (lt_forward_skip); ``perturb_layers`` (plain
        forward only): the blocks whose self-attention map is the identity (lt_forward_perturb); ``blur_layers`` (plain forward only,
        not beside ``perturb_layers``): the blocks whose self-attention reads queries blurred at width ``blur_sigma`` (lt_forward_blur, DESIGN
        7t); all empty: the call it was"""
        x, t32, out = self._eval_io(x, t)
        a = self._step_args(x, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        skip = self._skip_array(skip_layers, "forward")
        perturb = self._skip_array(perturb_layers, "forward", "perturb")
        blur = self._skip_array(blur_layers, "forward", "blur")
        if len(blur):
            if use_cfg:
                raise LuminaLibError("forward: blur_layers belongs to the plain forward (guided: forward_cfg_seg)")
            if len(perturb):
                raise LuminaLibError("forward: blur_layers together with perturb_layers is not served")
            if blur_sigma is None:
                raise LuminaLibError("forward: blur_layers needs blur_sigma (> 0; inf: the mean query)")
            name, layers = "lt_forward_blur", (skip, len(skip), blur, len(blur), float(blur_sigma))
        elif len(perturb):
            if use_cfg:
                raise LuminaLibError("forward: perturb_layers belongs to the plain forward (guided: forward_cfg_pag)")
            name, layers = "lt_forward_perturb", (skip, len(skip), perturb, len(perturb))
        elif len(skip):
            if use_cfg:
                raise LuminaLibError("forward: skip_layers belongs to the plain forward (guided: forward_cfg_slg)")
            name, layers = "lt_forward_skip", (skip, len(skip))
        else:
            name, layers = "lt_forward_cfg" if use_cfg else "lt_forward", ()
        self._call(name, self._dev(x), self._dev(t32), self._dev(out), C.byref(a), *layers, self._stream())
        return out

    def forward_packed(self, xs, t: torch.Tensor, *, scale_factor: float = 1.0, scale_watershed: float = 0.0,
                       base_seqlen: Optional[int] = None, proportional_attn: bool = False):
        """NextDiT.forward on a LIST of [C, H_b, W_b] latents (reference model.py:789-834): one padded batch on the engine,
        one output tensor per sample (lt_forward_packed)."""
        xs = [x.contiguous() for x in xs]
        for x in xs:
            _require_gpu(x, "x")
            if x.dim() != 3 or x.dtype != xs[0].dtype or x.device != xs[0].device:
                raise LuminaLibError("packed forward: every sample must be a [C, H, W] tensor of one dtype on one device")
        B = len(xs)
        t32 = t.to(device=xs[0].device, dtype=torch.float32).contiguous()
        outs = [torch.empty((self.in_channels,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device) for x in xs]
        a = self._step_args(xs[0].unsqueeze(0), 1.0, scale_factor, scale_watershed, base_seqlen, proportional_attn)
        a.batch, a.latent_h, a.latent_w = B, 0, 0
        xp = (C.c_void_p * B)(*[self._dev(x) for x in xs])
        op = (C.c_void_p * B)(*[self._dev(o) for o in outs])
        hw = (C.c_int32 * (2 * B))(*[v for x in xs for v in x.shape[1:]])
        self._call("lt_forward_packed", xp, hw, self._dev(t32), op, C.byref(a), self._stream())
        return outs

    def _pack(self, xs, what: str):
        """a list of [C, H_b, W_b] samples as ONE flat buffer in the engine's packed layout (sample b at element offset
        sum_{j<b} C H_j W_j), the host size list [B][2] and the (offset, shape) of every sample"""
        xs = list(xs)
        if not xs:
            raise LuminaLibError(f"{what}: empty sample list")
        for x in xs:
            _require_gpu(x, "x")
            if x.dim() != 3 or x.shape[0] != self.in_channels or x.dtype != xs[0].dtype or x.device != xs[0].device:
                raise LuminaLibError(f"{what}: every sample must be a [{self.in_channels}, H, W] tensor of one dtype on one device")
        flat = torch.cat([x.reshape(-1) for x in xs])
        hw = (C.c_int32 * (2 * len(xs)))(*[int(v) for x in xs for v in x.shape[1:]])
        spans, off = [], 0
        for x in xs:
            spans.append((off, tuple(x.shape)))
            off += x.numel()
        return flat, hw, spans

    def _packed_step_args(self, flat: torch.Tensor, B: int, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn) -> LtStepArgs:
        a = self._step_args(flat.view(1, 1, 1, -1), cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn)
        a.batch, a.latent_h, a.latent_w = B, 0, 0
        return a

    def forward_cfg_packed(self, xs, t: torch.Tensor, *, cfg_scale: float = 1.0, scale_factor: float = 1.0, scale_watershed: float = 1.0,
                           base_seqlen: Optional[int] = None, proportional_attn: bool = False):
        """forward_with_cfg on a LIST of 2 B' samples ``[C, H_b, W_b]`` with ``xs[b].shape == xs[b + B'].shape`` (lt_forward_cfg_packed): the
        reference's list ``forward`` on ``[x_0 .. x_{B'-1}] * 2`` followed by the guidance expression of model.py:901-913 per sample.
        Returns a list of 2 B' tensors, views of one allocation."""
        flat, hw, spans = self._pack(xs, "forward_cfg_packed")
        t32 = t.to(device=flat.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(flat)
        a = self._packed_step_args(flat, len(spans), cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn)
        self._call("lt_forward_cfg_packed", self._dev(flat), hw, self._dev(t32), self._dev(out), C.byref(a), self._stream())
        return self._unpacked(out, spans)

    # ---- whole trajectory -------------------------------------------------------------------------
    def sample_ode(self, z: torch.Tensor, tgrid: torch.Tensor, method: str, *, use_cfg: bool, cfg_scale: float = 1.0,
                   scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                   proportional_attn: bool = False, t_round_to_state_dtype: bool = True,
                   return_trajectory: bool = True, ntk_factor: float = 1.0) -> torch.Tensor:
        _require_gpu(z, "z")
        garr, n, code, _ = self._fixed_grid(method, tgrid)
        z = z.contiguous()
        a = self._step_args(z, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, n, z.shape, return_trajectory)
        self._call("lt_sample_ode", self._dev(z), traj_ptr, fin_ptr, garr, n, code, int(use_cfg), int(t_round_to_state_dtype), C.byref(a),
                   self._stream())
        return out

    def sample_ode_cached(self, z: torch.Tensor, tgrid, method: str, *, use_cfg: bool, threshold: float, coefficients=(0.0, 0.0, 0.0, 1.0, 0.0),
                          cfg_scale: float = 1.0, scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                          proportional_attn: bool = False, t_round_to_state_dtype: bool = True, return_trajectory: bool = True,
                          ntk_factor: float = 1.0):
        """``sample_ode`` under step caching (lt_sample_ode_cached): an evaluation whose modulated first-block input barely moved
        leaves the block stack out and adds the residual the stack produced the last time it ran.  ``transport.cache.sample_teacache`` is the
        definition.  Returns ``(states or last state, stats [ncalls, 3] float64: rel, acc after the add, ran)``."""
        from .transport.cache import check_cache_args
        if not isinstance(z, torch.Tensor):
            raise LuminaLibError("sample_ode_cached: a packed batch (a list of latents) is not served by step caching")
        _require_gpu(z, "z")
        garr, n, code, ncalls = self._fixed_grid(
            method, tgrid, f"sample_ode_cached: step caching is built for the fixed-grid methods {sorted(_lib.ODE_METHODS)}, not '{method}' "
                           "(the multistep and adaptive solvers are not served)")
        thr, coef = _refusing(check_cache_args, threshold, coefficients, who="sample_ode_cached")
        z = z.contiguous()
        a = self._step_args(z, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, n, z.shape, return_trajectory)
        stats = (C.c_double * (3 * max(ncalls, 1)))()
        self._call("lt_sample_ode_cached", self._dev(z), traj_ptr, fin_ptr, garr, n, code, int(use_cfg), int(t_round_to_state_dtype),
                   C.byref(a), thr, (C.c_double * 5)(*coef), stats, self._stream())
        return out, torch.tensor(stats[:3 * ncalls], dtype=torch.float64).reshape(ncalls, 3)

    def forward_cached(self, x: torch.Tensor, t: torch.Tensor, mode: str, *, use_cfg: bool, cfg_scale: float = 1.0, scale_factor: float = 1.0,
                       scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False, ntk_factor: float = 1.0):
        """one evaluation under step caching in its parts (lt_forward_cached).  ``mode`` ``"probe"``: the head of the evaluation; returns the
        indicator sums ``(S1, S0)`` against the previous probe.  ``"run"`` / ``"reuse"``: the rest of the evaluation that was probed last -
        the block stack (result: ``forward``'s, the residual kept) or the kept residual in its place; returns the output."""
        modes = {"probe": _lib.LT_CACHE_PROBE, "run": _lib.LT_CACHE_RUN, "reuse": _lib.LT_CACHE_REUSE}
        if mode not in modes:
            raise LuminaLibError(f"forward_cached: mode '{mode}' not in {sorted(modes)}")
        if not isinstance(x, torch.Tensor):
            raise LuminaLibError("forward_cached: a packed batch (a list of latents) is not served by step caching")
        x, t32, out = self._eval_io(x, t, writes=mode != "probe")
        a = self._step_args(x, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        sums = (C.c_double * 2)()
        self._call("lt_forward_cached", self._dev(x), self._dev(t32), self._dev(out), modes[mode], int(use_cfg), C.byref(a), sums,
                   self._stream())
        return (float(sums[0]), float(sums[1])) if mode == "probe" else out

    def last_cache_hits(self) -> int:
        """the evaluations of the last ``sample_ode_cached`` call that reused the residual"""
        return int(self.lib.lt_last_cache_hits(self.handle))

    def sample_ode_packed(self, zs, tgrid, method: str, *, use_cfg: bool, cfg_scale: float = 1.0, scale_factor: float = 1.0,
                          scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                          t_round_to_state_dtype: bool = True, return_trajectory: bool = True):
        """the fixed-grid trajectory of a LIST of differently sized latents in ONE call (lt_sample_ode_packed): every evaluation is the packed
        forward_with_cfg (``use_cfg``: 2 B' samples, halves of equal sizes) or the packed forward.  Returns one tensor per sample -
        ``[n_grid, C, H_b, W_b]`` or the last state ``[C, H_b, W_b]`` - all views of one allocation."""
        garr, n, code, _ = self._fixed_grid(method, tgrid)
        flat, hw, spans = self._pack(zs, "sample_ode_packed")
        a = self._packed_step_args(flat, len(spans), cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn)
        out, traj_ptr, fin_ptr = _traj_or_final(flat, n, flat.shape, return_trajectory)
        self._call("lt_sample_ode_packed", self._dev(flat), hw, traj_ptr, fin_ptr, garr, n, code, int(use_cfg), int(t_round_to_state_dtype),
                   C.byref(a), self._stream())
        return self._unpacked(out, spans, n if return_trajectory else None)

    # ---- inpainting: the fixed-grid trajectory with a per-element blend after every step -------------
    @staticmethod
    def _masked_operands(state: torch.Tensor, mask, x1, noise, what: str):
        """mask / source / noise as the engine reads them: the state's shape, dtype and device, contiguous (the callers broadcast)"""
        ops = []
        for name, v in (("mask", mask), ("x1", x1), ("noise", noise)):
            if not isinstance(v, torch.Tensor):
                raise LuminaLibError(f"{what}: {name} must be a tensor of the state's shape {tuple(state.shape)}")
            if tuple(v.shape) != tuple(state.shape) or v.dtype != state.dtype or v.device != state.device:
                raise LuminaLibError(f"{what}: {name} {tuple(v.shape)} {v.dtype} on {v.device} does not have the layout and dtype of the state "
                                     f"{tuple(state.shape)} {state.dtype} on {state.device}")
            ops.append(v.contiguous())
        return ops

    @staticmethod
    def _refuse_masked_multistep(method: str, what: str) -> None:
        if method in _lib.ODE_MULTISTEP_METHODS:
            from .transport.multistep import MASKED_REFUSAL
            raise LuminaLibError(f"{what}: {MASKED_REFUSAL.format(method)}")

    def sample_ode_masked(self, z: torch.Tensor, tgrid, mask: torch.Tensor, x1: torch.Tensor, noise: torch.Tensor, method: str, *, use_cfg: bool,
                          cfg_scale: float = 1.0, scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                          proportional_attn: bool = False, t_round_to_state_dtype: bool = True, return_trajectory: bool = True,
                          ntk_factor: float = 1.0) -> torch.Tensor:
        """``sample_ode`` with the inpainting blend after every full step (lt_sample_ode_masked): ``mask`` (1 = generate, 0 = keep), the
        source latent ``x1`` and the ``noise`` the trajectory started from, all shaped and typed like ``z``"""
        _require_gpu(z, "z")
        self._refuse_masked_multistep(method, "sample_ode_masked")
        garr, n, code, _ = self._fixed_grid(method, tgrid)
        z = z.contiguous()
        m, src, nz = self._masked_operands(z, mask, x1, noise, "sample_ode_masked")
        a = self._step_args(z, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, n, z.shape, return_trajectory)
        self._call("lt_sample_ode_masked", self._dev(z), self._dev(m), self._dev(src), self._dev(nz), traj_ptr, fin_ptr, garr, n, code,
                   int(use_cfg), int(t_round_to_state_dtype), C.byref(a), self._stream())
        return out

    def sample_ode_masked_packed(self, zs, tgrid, masks, x1s, noises, method: str, *, use_cfg: bool, cfg_scale: float = 1.0,
                                 scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                                 proportional_attn: bool = False, t_round_to_state_dtype: bool = True, return_trajectory: bool = True):
        """``sample_ode_packed`` with the inpainting blend (lt_sample_ode_masked_packed): ``masks``, ``x1s`` and ``noises`` are lists like
        ``zs``, sample b of each shaped like ``zs[b]``"""
        self._refuse_masked_multistep(method, "sample_ode_masked_packed")
        garr, n, code, _ = self._fixed_grid(method, tgrid)
        zs = list(zs)
        flat, hw, spans = self._pack(zs, "sample_ode_masked_packed")
        flats = []
        for name, vs in (("mask", masks), ("x1", x1s), ("noise", noises)):
            vs = list(vs)
            if len(vs) != len(zs) or any(not isinstance(v, torch.Tensor) or tuple(v.shape) != tuple(z.shape) or v.dtype != z.dtype
                                         or v.device != z.device for v, z in zip(vs, zs)):
                raise LuminaLibError(f"sample_ode_masked_packed: {name} must be a list of {len(zs)} tensors, each with the shape, dtype and "
                                     "device of its sample")
            flats.append(torch.cat([v.reshape(-1) for v in vs]))
        a = self._packed_step_args(flat, len(spans), cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn)
        out, traj_ptr, fin_ptr = _traj_or_final(flat, n, flat.shape, return_trajectory)
        self._call("lt_sample_ode_masked_packed", self._dev(flat), hw, *[self._dev(f) for f in flats], traj_ptr, fin_ptr, garr, n, code,
                   int(use_cfg), int(t_round_to_state_dtype), C.byref(a), self._stream())
        return self._unpacked(out, spans, n if return_trajectory else None)

    # ---- guidance schedules: a scale per stage, conditional-only stages at half the rows -------------
    def sample_ode_cfg_schedule(self, z: torch.Tensor, tgrid, table, method: str, *, scale_factor: float = 1.0, scale_watershed: float = 1.0,
                                base_seqlen: Optional[int] = None, proportional_attn: bool = False, t_round_to_state_dtype: bool = True,
                                return_trajectory: bool = True, ntk_factor: float = 1.0, cfg_scale=None) -> torch.Tensor:
        """``sample_ode`` with guidance whose scale is ``table[i * stages + k]`` at stage k of interval i (lt_sample_ode_cfg_schedule): stages
        at scale 1 exactly evaluate the ``z.size(0) / 2`` cond rows alone.  ``table``: ``(len(tgrid) - 1) * stages`` fp32 values (a tensor or a
        sequence; ``transport.guidance.cfg_table`` builds one).  The conditioning was prepared for all rows, once.  ``cfg_scale`` is ignored."""
        _require_gpu(z, "z")
        garr, n, code, count = self._fixed_grid(method, tgrid)
        z = z.contiguous()
        tab = self._stage_table(table, "sample_ode_cfg_schedule", n, method, count)
        a = self._step_args(z, 0.0, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, max(n, 1), z.shape, return_trajectory)
        self._call("lt_sample_ode_cfg_schedule", self._dev(z), traj_ptr, fin_ptr, garr, n, code, self._host(tab), int(t_round_to_state_dtype),
                   C.byref(a), self._stream())
        return out

    # ---- skip-layer guidance: a third prediction with a set of blocks left out -------------
    @staticmethod
    def _skip_array(skip_layers, what: str, kind: str = "skip"):
        """the layer set as a ctypes int32 array (its contents are the C entry's to check)"""
        if isinstance(skip_layers, torch.Tensor):
            skip_layers = skip_layers.reshape(-1).tolist()
        idx = list(skip_layers) if skip_layers is not None else []
        for v in idx:
            if isinstance(v, bool) or int(v) != v:
                raise LuminaLibError(f"{what}: {kind} layer {v!r} is not an integer index")
        return (C.c_int32 * len(idx))(*[int(v) for v in idx])

    def forward_cfg_slg(self, x: torch.Tensor, t: torch.Tensor, *, cfg_scale: float, slg_scale: float, slg_layers, scale_factor: float = 1.0,
                        scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                        ntk_factor: float = 1.0) -> torch.Tensor:
        """one guided evaluation with skip-layer guidance (lt_forward_cfg_slg): ``u + w (c - u) + s (c - k)`` on the guided channels, ``k`` the
        cond rows evaluated with the blocks ``slg_layers`` left out.  ``slg_scale == 0`` is ``forward(use_cfg=True)``."""
        x, t32, out = self._eval_io(x, t)
        a = self._step_args(x, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        skip = self._skip_array(slg_layers, "forward_cfg_slg")
        self._call("lt_forward_cfg_slg", self._dev(x), self._dev(t32), self._dev(out), float(cfg_scale), float(slg_scale), skip, len(skip),
                   C.byref(a), self._stream())
        return out

    # ---- perturbed-attention guidance: the third prediction runs a set of blocks with the identity as their attention map -----
    def forward_cfg_pag(self, x: torch.Tensor, t: torch.Tensor, *, cfg_scale: float, pag_scale: float, pag_layers, skip_layers=(),
                        scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                        proportional_attn: bool = False, ntk_factor: float = 1.0) -> torch.Tensor:
        """one guided evaluation with perturbed-attention guidance (lt_forward_cfg_pag): ``u + w (c - u) + s (c - p)`` on the guided channels,
        ``p`` the cond rows evaluated with the blocks ``pag_layers`` perturbed (and ``skip_layers`` left out).  ``pag_scale == 0`` is
        ``forward(use_cfg=True)``."""
        x, t32, out = self._eval_io(x, t)
        a = self._step_args(x, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        skip = self._skip_array(skip_layers, "forward_cfg_pag")
        perturb = self._skip_array(pag_layers, "forward_cfg_pag", "perturb")
        self._call("lt_forward_cfg_pag", self._dev(x), self._dev(t32), self._dev(out), float(cfg_scale), float(pag_scale), skip, len(skip),
                   perturb, len(perturb), C.byref(a), self._stream())
        return out

    # ---- smoothed-energy guidance: the third prediction runs a set of blocks on Gaussian-blurred queries -----
    def forward_cfg_seg(self, x: torch.Tensor, t: torch.Tensor, *, cfg_scale: float, seg_scale: float, seg_layers, seg_sigma: float,
                        skip_layers=(), scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                        proportional_attn: bool = False, ntk_factor: float = 1.0) -> torch.Tensor:
        """one guided evaluation with smoothed-energy guidance (lt_forward_cfg_seg): ``u + w (c - u) + s (c - b)`` on the guided channels,
        ``b`` the cond rows evaluated with the queries of the blocks ``seg_layers`` blurred at width ``seg_sigma`` (and ``skip_layers`` left
        out).  ``seg_scale == 0`` is ``forward(use_cfg=True)``."""
        x, t32, out = self._eval_io(x, t)
        a = self._step_args(x, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        skip = self._skip_array(skip_layers, "forward_cfg_seg")
        blur = self._skip_array(seg_layers, "forward_cfg_seg", "blur")
        self._call("lt_forward_cfg_seg", self._dev(x), self._dev(t32), self._dev(out), float(cfg_scale), float(seg_scale), skip, len(skip),
                   blur, len(blur), float(seg_sigma), C.byref(a), self._stream())
        return out

    def sample_ode_cfg_seg(self, z: torch.Tensor, tgrid, table, seg, seg_layers, seg_sigma: float, method: str, *, skip_layers=(),
                           **kw) -> torch.Tensor:
        """``sample_ode_cfg_pag`` with the third prediction taken with the queries of the blocks ``seg_layers`` blurred at width ``seg_sigma``
        (lt_sample_ode_cfg_seg).  ``transport.guidance.sample_cfg_seg`` is the definition."""
        return self._sample_ode_cfg_third("sample_ode_cfg_seg", z, tgrid, table, seg, skip_layers, seg_layers, method, seg_sigma=seg_sigma, **kw)

    def sample_ode_cfg_pag(self, z: torch.Tensor, tgrid, table, pag, pag_layers, method: str, *, skip_layers=(), **kw) -> torch.Tensor:
        """``sample_ode_cfg_slg`` with the third prediction taken with the blocks ``pag_layers`` perturbed and ``skip_layers`` left out, under
        the one scale table ``pag`` (lt_sample_ode_cfg_pag).  ``transport.guidance.sample_cfg_pag`` is the definition."""
        return self._sample_ode_cfg_third("sample_ode_cfg_pag", z, tgrid, table, pag, skip_layers, pag_layers, method, **kw)

    def sample_ode_cfg_slg(self, z: torch.Tensor, tgrid, table, slg, slg_layers, method: str, *, scale_factor: float = 1.0,
                           scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                           t_round_to_state_dtype: bool = True, return_trajectory: bool = True, ntk_factor: float = 1.0,
                           cfg_scale=None) -> torch.Tensor:
        """``sample_ode_cfg_schedule`` with a skip-layer scale per stage (lt_sample_ode_cfg_slg): a stage with ``slg != 0`` also evaluates the
        cond rows with the blocks ``slg_layers`` left out and pushes the guided output away from that prediction.
        ``transport.guidance.sample_cfg_slg`` is the definition, ``slg_table`` builds the scale tables."""
        return self._sample_ode_cfg_third("sample_ode_cfg_slg", z, tgrid, table, slg, slg_layers, None, method, scale_factor=scale_factor,
                                          scale_watershed=scale_watershed, base_seqlen=base_seqlen, proportional_attn=proportional_attn,
                                          t_round_to_state_dtype=t_round_to_state_dtype, return_trajectory=return_trajectory,
                                          ntk_factor=ntk_factor, cfg_scale=cfg_scale)

    def _sample_ode_cfg_third(self, who: str, z, tgrid, table, third, skip_layers, pag_layers, method: str, *, scale_factor: float = 1.0,
                              scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                              t_round_to_state_dtype: bool = True, return_trajectory: bool = True, ntk_factor: float = 1.0,
                              cfg_scale=None, seg_sigma=None) -> torch.Tensor:
        """the guided trajectory with a third prediction per stage under the scale table ``third``: the cond rows with ``skip_layers`` left
        out (``pag_layers=None``: lt_sample_ode_cfg_slg) or, besides, ``pag_layers`` perturbed (lt_sample_ode_cfg_pag) or - ``seg_sigma``
        given - run on queries blurred at that width (lt_sample_ode_cfg_seg)"""
        what, short = ("skip-layer guidance", "slg") if pag_layers is None else ("perturbed-attention guidance", "pag")
        if seg_sigma is not None:
            what, short = "smoothed-energy guidance", "seg"
        if isinstance(z, (list, tuple)):
            raise LuminaLibError(f"{who}: a packed batch (a list of latents) is not served")
        _require_gpu(z, "z")
        garr, n, code, count = self._fixed_grid(
            method, tgrid, f"{who}: {what} is built for the fixed-grid methods {sorted(_lib.ODE_METHODS)}, not '{method}'")
        z = z.contiguous()
        # (third=None: the C entry refuses the null table by name)
        sl = None if third is None else self._table(
            third, count, lambda got: f"{who}: the {short} table has {got} entries, the grid has {count} evaluations")
        tab = self._table(table, count, lambda got: f"{who}: the guidance table has {got} entries, the grid has {count} evaluations")
        skip = self._skip_array(skip_layers, who)
        a = self._step_args(z, 0.0, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, max(n, 1), z.shape, return_trajectory)
        layers = (skip, len(skip))
        if pag_layers is not None:
            perturb = self._skip_array(pag_layers, who, "blur" if seg_sigma is not None else "perturb")
            layers += (perturb, len(perturb))
        if seg_sigma is not None:
            layers += (float(seg_sigma),)
        self._call(f"lt_sample_ode_cfg_{short}", self._dev(z), traj_ptr, fin_ptr, garr, n, code, self._host(tab), self._host(sl), *layers,
                   int(t_round_to_state_dtype), C.byref(a), self._stream())
        return out

    # ---- rescaled and norm-limited guidance: a per-sample factor on every guided stage -------------
    @staticmethod
    def _rule(rescale, norm_limit, what: str):
        from .transport.guidance import check_rule
        return _refusing(check_rule, rescale, norm_limit, who=what)

    def sample_ode_cfg_rule(self, z: torch.Tensor, tgrid, table, method: str, *, rescale: float = 0.0, norm_limit: float = math.inf,
                            scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                            proportional_attn: bool = False, t_round_to_state_dtype: bool = True, return_trajectory: bool = True,
                            ntk_factor: float = 1.0, cfg_scale=None) -> torch.Tensor:
        """``sample_ode_cfg_schedule`` whose guided stages multiply their guided channels by the per-sample factor of
        ``transport.guidance.guided_rule`` (lt_sample_ode_cfg_rule): ``rescale`` in [0, 1] pulls the guided output's std towards the conditional
        output's, ``norm_limit`` (> 0, inf: off) caps its L2 norm at that multiple of the conditional output's.  Stages at scale 1 exactly are
        conditional-only and skip the rule.  This IS the rule call, at any parameters; ``model.sample_ode_cfg_schedule`` routes the defaults to
        the schedule call."""
        _require_gpu(z, "z")
        garr, n, code, count = self._fixed_grid(method, tgrid)
        rescale, norm_limit = self._rule(rescale, norm_limit, "sample_ode_cfg_rule")
        z = z.contiguous()
        tab = self._stage_table(table, "sample_ode_cfg_rule", n, method, count)
        a = self._step_args(z, 0.0, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, max(n, 1), z.shape, return_trajectory)
        self._call("lt_sample_ode_cfg_rule", self._dev(z), traj_ptr, fin_ptr, garr, n, code, self._host(tab), rescale, norm_limit,
                   int(t_round_to_state_dtype), C.byref(a), self._stream())
        return out

    def forward_cfg_rule(self, x: torch.Tensor, t: torch.Tensor, *, cfg_scale: float, rescale: float = 0.0, norm_limit: float = math.inf,
                         scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                         proportional_attn: bool = False, ntk_factor: float = 1.0) -> torch.Tensor:
        """one guided evaluation at ``cfg_scale`` under the rule (lt_forward_cfg_rule): ``guided_rule`` on the model's output of all rows"""
        x, t32, out = self._eval_io(x, t)
        rescale, norm_limit = self._rule(rescale, norm_limit, "forward_cfg_rule")
        a = self._step_args(x, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        self._call("lt_forward_cfg_rule", self._dev(x), self._dev(t32), self._dev(out), rescale, norm_limit, C.byref(a), self._stream())
        return out

    # ---- projected guidance: APG and CFG-Zero*  -------------
    @staticmethod
    def _project(apg, zero_star, zero_init, what: str, n_grid=None):
        from .transport.guidance import check_project
        form, eta, beta, r, zero_init = _refusing(check_project, apg, zero_star, zero_init, n_grid=n_grid, who=what)
        if form is None:
            raise LuminaLibError(f"{what}: needs a projected form - apg=dict(eta=, momentum=, norm_threshold=) or zero_star=True")
        return _lib.PROJECT_FORMS[form], eta, beta, r, zero_init

    def sample_ode_cfg_project(self, z: torch.Tensor, tgrid, table, method: str, *, apg=None, zero_star: bool = False, zero_init: int = 0,
                               scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                               proportional_attn: bool = False, t_round_to_state_dtype: bool = True, return_trajectory: bool = True,
                               ntk_factor: float = 1.0, cfg_scale=None) -> torch.Tensor:
        """``sample_ode_cfg_schedule`` whose guided stages form their output by ``transport.guidance.guided_project``
        (lt_sample_ode_cfg_project): ``apg=dict(eta=, momentum=, norm_threshold=)`` - the update ``c - u`` with momentum, a norm clip and its
        part parallel to ``c`` damped by ``eta`` - or ``zero_star=True`` - the unconditional row rescaled by ``<c, u> / <u, u>``, with
        ``zero_init`` grid intervals of zero velocity at the start, for which nothing is evaluated.  Stages at scale 1 exactly are
        conditional-only.  ``transport.guidance.sample_cfg_project`` is the definition."""
        if isinstance(z, (list, tuple)):
            raise LuminaLibError("sample_ode_cfg_project: a packed batch (a list of latents) is not served")
        _require_gpu(z, "z")
        garr, n, code, count = self._fixed_grid(
            method, tgrid, f"sample_ode_cfg_project: projected guidance is built for the fixed-grid methods {sorted(_lib.ODE_METHODS)}, "
                           f"not '{method}'")
        z = z.contiguous()
        form, eta, beta, r, zero_init = self._project(apg, zero_star, zero_init, "sample_ode_cfg_project", n_grid=n)
        tab = self._stage_table(table, "sample_ode_cfg_project", n, method, count)
        a = self._step_args(z, 0.0, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, max(n, 1), z.shape, return_trajectory)
        self._call("lt_sample_ode_cfg_project", self._dev(z), traj_ptr, fin_ptr, garr, n, code, self._host(tab), form, eta, beta, r, zero_init,
                   int(t_round_to_state_dtype), C.byref(a), self._stream())
        return out

    def forward_cfg_project(self, x: torch.Tensor, t: torch.Tensor, *, cfg_scale: float, apg=None, zero_star: bool = False,
                            keep_momentum: bool = False, scale_factor: float = 1.0, scale_watershed: float = 1.0,
                            base_seqlen: Optional[int] = None, proportional_attn: bool = False, ntk_factor: float = 1.0) -> torch.Tensor:
        """one guided evaluation at ``cfg_scale`` under a projected form (lt_forward_cfg_project): ``guided_project`` on the model's output of
        all rows.  ``keep_momentum`` (APG): continue from the momentum the last projected evaluation of this shape left, instead of zero."""
        if isinstance(x, (list, tuple)):
            raise LuminaLibError("forward_cfg_project: a packed batch (a list of latents) is not served")
        x, t32, out = self._eval_io(x, t)
        form, eta, beta, r, _ = self._project(apg, zero_star, 0, "forward_cfg_project")
        a = self._step_args(x, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        self._call("lt_forward_cfg_project", self._dev(x), self._dev(t32), self._dev(out), form, eta, beta, r, int(bool(keep_momentum)),
                   C.byref(a), self._stream())
        return out

    # ---- guidance reuse: the cond - uncond difference taken on refresh stages, reused on half-row stages -------------
    @classmethod
    def _reuse_tables(cls, table, reuse, count: int, what: str):
        """the scale table and the flag table as contiguous fp32 / int32 CPU tensors of ``count`` entries (their contents are the C entry's to
        check)"""
        tab = cls._table(table)
        if reuse is None:
            raise LuminaLibError(f"{what}: reuse is None (one 0 / 1 flag per evaluation; transport.guidance.cfg_reuse_table builds one)")
        flg = reuse if isinstance(reuse, torch.Tensor) else torch.tensor(list(reuse))
        if flg.is_floating_point() and not bool((flg == flg.round()).all()):
            raise LuminaLibError(f"{what}: a reuse flag is not 0 (refresh) or 1 (reuse)")
        flg = cls._table(flg, dtype=torch.int32)
        if tab.numel() != count or flg.numel() != count:
            raise LuminaLibError(f"{what}: the guidance table has {tab.numel()} entries and the reuse table {flg.numel()}, the grid has {count} "
                                 "evaluations")
        return tab, flg

    def sample_ode_cfg_reuse(self, z: torch.Tensor, tgrid, table, reuse, method: str, *, scale_factor: float = 1.0, scale_watershed: float = 1.0,
                             base_seqlen: Optional[int] = None, proportional_attn: bool = False, t_round_to_state_dtype: bool = True,
                             return_trajectory: bool = True, ntk_factor: float = 1.0, cfg_scale=None) -> torch.Tensor:
        """``sample_ode_cfg_schedule`` with a flag per stage (lt_sample_ode_cfg_reuse): a guided stage with flag 0 evaluates all rows and keeps
        the cond - uncond difference of its guided channels, one with flag 1 evaluates the ``z.size(0) / 2`` cond rows alone and guides them
        with the difference kept.  ``transport.guidance.sample_cfg_reuse`` is the definition, ``cfg_reuse_table`` builds flag tables."""
        if isinstance(z, (list, tuple)):
            raise LuminaLibError("sample_ode_cfg_reuse: a packed batch (a list of latents) is not served")
        _require_gpu(z, "z")
        garr, n, code, count = self._fixed_grid(method, tgrid)
        z = z.contiguous()
        tab, flg = self._reuse_tables(table, reuse, count, "sample_ode_cfg_reuse")
        a = self._step_args(z, 0.0, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, max(n, 1), z.shape, return_trajectory)
        self._call("lt_sample_ode_cfg_reuse", self._dev(z), traj_ptr, fin_ptr, garr, n, code, self._host(tab), self._host(flg),
                   int(t_round_to_state_dtype), C.byref(a), self._stream())
        return out

    def sample_ode_multistep_cfg_reuse(self, z: torch.Tensor, tgrid, method: Optional[str], table, reuse, *, coef=None, scale_factor: float = 1.0,
                                       scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                                       t_round_to_state_dtype: bool = True, return_trajectory: bool = True, ntk_factor: float = 1.0,
                                       cfg_scale=None) -> torch.Tensor:
        """``sample_ode_multistep`` with a guidance scale and a reuse flag per evaluation (lt_sample_ode_multistep_cfg_reuse);
        ``transport.guidance.sample_cfg_reuse_multistep`` is the definition."""
        _require_gpu(z, "z")
        z = z.contiguous()
        garr, n = _grid_array(tgrid)
        coef, corrector = self._multistep_table(tgrid, method, n, "sample_ode_multistep_cfg_reuse", coef)
        tab, flg = self._reuse_tables(table, reuse, n - 1, "sample_ode_multistep_cfg_reuse")
        a = self._step_args(z, 0.0, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, n, z.shape, return_trajectory)
        self._call("lt_sample_ode_multistep_cfg_reuse", self._dev(z), traj_ptr, fin_ptr, garr, n, self._host(coef), corrector, self._host(tab),
                   self._host(flg), int(t_round_to_state_dtype), C.byref(a), self._stream())
        return out

    def forward_cfg_reuse(self, x: torch.Tensor, t: torch.Tensor, *, cfg_scale: float, reuse: bool = False, scale_factor: float = 1.0,
                          scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                          ntk_factor: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one guided evaluation at ``cfg_scale`` (lt_forward_cfg_reuse): ``reuse=False`` is ``forward_with_cfg`` and keeps the cond - uncond
        difference, ``reuse=True`` evaluates the cond rows alone and guides them with the difference kept - refused by name when none of this
        shape is there.  ``out`` (optional): the tensor to write, shaped and typed like ``x``."""
        x, t32, out = self._eval_io(x, t, out=out)
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
            raise LuminaLibError("forward_cfg_reuse: out must be contiguous and shaped and typed like x")
        a = self._step_args(x, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        self._call("lt_forward_cfg_reuse", self._dev(x), self._dev(t32), self._dev(out), int(bool(reuse)), C.byref(a), self._stream())
        return out

    # ---- linear multistep sampling: one evaluation per interval -------------
    @staticmethod
    def _multistep_table(tgrid, method: str, n: int, what: str, coef=None):
        """the weight table of ``transport.multistep`` for this grid as the engine reads it, and whether the corrector halves are used;
        ``coef``: the caller's own fp32 ``[n - 1, 8]`` table instead (``multistep_odeint(..., table=)`` is its host loop)"""
        from .transport import multistep
        if coef is not None:
            tab = torch.as_tensor(coef).detach().to("cpu", torch.float32).contiguous()
            if tuple(tab.shape) != (max(n - 1, 0), 8):
                raise LuminaLibError(f"{what}: coef must be [{max(n - 1, 0)}, 8] (a_0..3, b_0..3 per interval), got {tuple(tab.shape)}")
            if n < 2:
                raise LuminaLibError(f"{what}: need at least 2 grid points")
            return tab, int(bool((tab[:, :4] != 0).any()))
        if method not in multistep.MULTISTEP_METHODS:
            raise LuminaLibError(f"{what}: multistep method '{method}' not in {list(multistep.MULTISTEP_METHODS)}")
        if n < 2:
            raise LuminaLibError(f"{what}: need at least 2 grid points")
        return _refusing(multistep.multistep_table, tgrid, method, who=what).contiguous(), int(multistep.is_corrector(method))

    def sample_ode_multistep(self, z: torch.Tensor, tgrid, method: Optional[str], *, use_cfg: bool, cfg_scale: float = 1.0, table=None, coef=None,
                             rescale: float = 0.0,
                             norm_limit: float = math.inf, scale_factor: float = 1.0, scale_watershed: float = 1.0,
                             base_seqlen: Optional[int] = None, proportional_attn: bool = False, t_round_to_state_dtype: bool = True,
                             return_trajectory: bool = True, ntk_factor: float = 1.0) -> torch.Tensor:
        """``ab2`` / ``ab3`` / ``abm2`` / ``abm3`` of ``transport.multistep`` in ONE call (lt_sample_ode_multistep): ``len(tgrid) - 1`` model
        evaluations, the weights from ``multistep_table``.  ``table`` (optional): a guidance scale per evaluation, ``len(tgrid) - 1`` values,
        as ``sample_ode_cfg_schedule`` takes one per stage; ``rescale`` / ``norm_limit``: the rule of ``sample_ode_cfg_rule`` on the guided
        evaluations.  ``coef`` (optional): the caller's own weight table ``[len(tgrid) - 1, 8]`` in place of the method's - the table is
        the contract (``method`` is then not read); a row whose corrector half is all 0 takes ``y_i = p_i``.  Returns all ``len(tgrid)``
        recorded states or the last one."""
        _require_gpu(z, "z")
        z = z.contiguous()
        garr, n = _grid_array(tgrid)
        coef, corrector = self._multistep_table(tgrid, method, n, "sample_ode_multistep", coef)
        rescale, norm_limit = self._rule(rescale, norm_limit, "sample_ode_multistep")
        tab = None if table is None else self._table(
            table, n - 1, lambda got: f"sample_ode_multistep: the guidance table has {got} entries, a {n}-point grid has {n - 1} evaluations")
        a = self._step_args(z, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out, traj_ptr, fin_ptr = _traj_or_final(z, n, z.shape, return_trajectory)
        self._call("lt_sample_ode_multistep", self._dev(z), traj_ptr, fin_ptr, garr, n, self._host(coef), corrector, self._host(tab), rescale,
                   norm_limit, int(use_cfg), int(t_round_to_state_dtype), C.byref(a), self._stream())
        return out

    def sample_ode_multistep_packed(self, zs, tgrid, method: str, *, use_cfg: bool, cfg_scale: float = 1.0, scale_factor: float = 1.0,
                                    scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                                    t_round_to_state_dtype: bool = True, return_trajectory: bool = True):
        """``sample_ode_multistep`` on a LIST of differently sized latents (lt_sample_ode_multistep_packed), every evaluation the packed
        forward_with_cfg (``use_cfg``) or the packed forward.  Returns one tensor per sample, all views of one allocation."""
        flat, hw, spans = self._pack(zs, "sample_ode_multistep_packed")
        garr, n = _grid_array(tgrid)
        coef, corrector = self._multistep_table(tgrid, method, n, "sample_ode_multistep_packed")
        a = self._packed_step_args(flat, len(spans), cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn)
        out, traj_ptr, fin_ptr = _traj_or_final(flat, n, flat.shape, return_trajectory)
        self._call("lt_sample_ode_multistep_packed", self._dev(flat), hw, traj_ptr, fin_ptr, garr, n, self._host(coef), corrector, int(use_cfg),
                   int(t_round_to_state_dtype), C.byref(a), self._stream())
        return self._unpacked(out, spans, n if return_trajectory else None)

    def sample_ode_adaptive(self, z: torch.Tensor, tgrid: torch.Tensor, method: str, *, rtol: float, atol: float,
                            first_step: Optional[float] = None, max_steps: int = 2 ** 31 - 1, use_cfg: bool, cfg_scale: float = 1.0,
                            scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None,
                            proportional_attn: bool = False, t_round_to_state_dtype: bool = True, ntk_factor: float = 1.0,
                            max_recorded_steps: int = 4096):
        """torchdiffeq's adaptive dopri5 / bosh3 / fehlberg2 / adaptive_heun in ONE call (lt_sample_ode_adaptive): the states at every point
        of ``tgrid`` ``[len(tgrid), *z.shape]`` and a dict ``nfe, accepted, rejected, first_step, dt`` (``dt``: the step size of every
        attempted step, the first ``max_recorded_steps`` of them).  ``first_step=None`` selects the first step by torchdiffeq's heuristic.
        Synchronises the stream once per attempted step (the host reads the error ratio)."""
        _require_gpu(z, "z")
        if method not in _lib.ODE_ADAPTIVE_METHODS:
            raise LuminaLibError(f"adaptive method '{method}' not in {sorted(_lib.ODE_ADAPTIVE_METHODS)}")
        z = z.contiguous()
        garr, n = _grid_array(tgrid)
        a = self._step_args(z, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        out = torch.empty((max(n, 1),) + tuple(z.shape), dtype=z.dtype, device=z.device)
        dts = (C.c_float * max_recorded_steps)()
        st = _lib.LtOdeAdaptiveStats(dt_cap=max_recorded_steps, dt_host=dts)
        self._call("lt_sample_ode_adaptive", self._dev(z), self._dev(out), garr, n, _lib.ODE_ADAPTIVE_METHODS[method], float(rtol), float(atol),
                   0.0 if first_step is None else float(first_step), int(min(max_steps, 2 ** 31 - 1)), int(use_cfg),
                   int(t_round_to_state_dtype), C.byref(a), self._stream(), C.byref(st))
        stats = dict(nfe=int(st.nfe), accepted=int(st.accepted), rejected=int(st.rejected), first_step=float(st.first_step),
                     dt=[float(dts[i]) for i in range(min(st.dt_count, max_recorded_steps))])
        return out, stats

    def sample_sde(self, z: torch.Tensor, noise: torch.Tensor, steps: torch.Tensor, last_coef: Optional[torch.Tensor], method: str,
                   last_step: Optional[str], *, use_cfg: bool, cfg_scale: float = 1.0, scale_factor: float = 1.0,
                   scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                   ntk_factor: float = 1.0) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Euler-Maruyama / Heun SDE sampling with a last-step rule in ONE call (lt_sample_sde; one model evaluation per stage).
        ``noise`` [n_steps - 1, *z.shape] on the device in the state dtype (the caller's draws), ``steps`` fp32 [(n_steps - 1) * stages,
        LT_SDE_REC] and ``last_coef`` fp32 [LT_SDE_REC] on the host (``transport.integrators.sde_table``).  Returns (loop states
        [n_steps - 1, *z.shape], last-step state) - the latter fp32 for "Mean" / "Tweedie" as in the reference, None for ``last_step=None``."""
        _require_gpu(z, "z")
        _require_gpu(noise, "noise")
        if method not in _lib.SDE_METHODS:
            raise LuminaLibError(f"SDE method '{method}' not in {sorted(_lib.SDE_METHODS)}")
        if last_step not in _lib.SDE_LAST_STEPS:
            raise LuminaLibError(f"SDE last step '{last_step}' not in {list(_lib.SDE_LAST_STEPS)}")
        z = z.contiguous()
        stages = 2 if method == "Heun" else 1
        steps = steps.detach().to("cpu", torch.float32).contiguous()
        if steps.dim() != 2 or steps.shape[1] != _lib.LT_SDE_REC or steps.shape[0] % stages:
            raise LuminaLibError(f"sample_sde: steps must be [(n_steps - 1) * {stages}, {_lib.LT_SDE_REC}], got {tuple(steps.shape)}")
        n_loop = steps.shape[0] // stages
        if noise.dtype != z.dtype or noise.device != z.device or tuple(noise.shape) != (n_loop,) + tuple(z.shape):
            raise LuminaLibError(f"sample_sde: noise must be {(n_loop,) + tuple(z.shape)} {z.dtype} on {z.device}, got {tuple(noise.shape)} "
                                 f"{noise.dtype} on {noise.device}")
        noise = noise.contiguous()
        a = self._step_args(z, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        traj = torch.empty_like(noise)
        final = last = None
        if last_step is not None:
            if last_coef is None:
                raise LuminaLibError("sample_sde: a last step needs its coefficient record")
            last = last_coef.detach().to("cpu", torch.float32).contiguous()
            if last.numel() != _lib.LT_SDE_REC:
                raise LuminaLibError(f"sample_sde: last_coef must hold {_lib.LT_SDE_REC} floats, got {last.numel()}")
            final = torch.empty_like(z, dtype=z.dtype if last_step == "Euler" else torch.float32)
        self._call("lt_sample_sde", self._dev(z), self._dev(noise), self._dev(traj), self._dev(final), self._host(steps), n_loop + 1,
                   _lib.SDE_METHODS[method], _lib.SDE_LAST_STEPS[last_step], self._host(last), int(use_cfg), C.byref(a), self._stream())
        return traj, final

    # ---- prompt-driven editing (FlowEdit) ---------------------------------------------------------------
    def sample_flowedit(self, x_src: torch.Tensor, tgrid, noise: torch.Tensor, scales, *, z: Optional[torch.Tensor] = None,
                        scale_factor: float = 1.0, scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                        ntk_factor: float = 1.0, cfg_channels: int = 3, return_trajectory: bool = True) -> torch.Tensor:
        """FlowEdit's inversion-free edit in ONE call (lt_sample_flowedit; ``transport.edit.sample_flowedit`` is the definition): the source
        ``x_src [B', C, H, W]``, the edit state ``z`` (default: ``x_src``), ``noise [len(tgrid) - 1, B', C, H, W]`` (the caller's draws) and the
        fp32 table ``scales [len(tgrid) - 1, 2]`` of ``(w_s, w_t)`` pairs (``transport.edit.flowedit_scales``).  Needs the conditioning prepared
        for 4 B' rows: source, target, negative source, negative target.  Returns ``[len(tgrid), B', C, H, W]`` or the last state."""
        from .transport.edit import check_edit_operands, check_scales
        _require_gpu(x_src, "x_src")
        garr, n = _grid_array(tgrid)
        if n < 2:
            raise LuminaLibError("sample_flowedit: need at least 2 grid points")
        x_src, z, noise = _refusing(check_edit_operands, x_src, z, noise, n - 1, who="sample_flowedit")
        sc = _refusing(check_scales, scales, n - 1, who="sample_flowedit")
        x_src, z, noise = x_src.contiguous(), z.contiguous(), noise.contiguous()
        a = self._step_args(x_src, 1.0, scale_factor, scale_watershed, base_seqlen, proportional_attn, cfg_channels=int(cfg_channels),
                            ntk_factor=ntk_factor)
        a.batch = 4 * x_src.shape[0]
        out, traj_ptr, fin_ptr = _traj_or_final(x_src, n, x_src.shape, return_trajectory)
        self._call("lt_sample_flowedit", self._dev(z), self._dev(x_src), self._dev(noise), traj_ptr, fin_ptr, garr, self._host(sc), n,
                   C.byref(a), self._stream())
        return out

    # ---- multi-view (visual-anagram) sampling -------------------------------------------------------------------
    def set_views(self, views, latent_h: int, latent_w: int) -> None:
        """upload the tables of a list of ``views.BaseView`` objects (or a ready ``(perm [V, h*w], vsign [V, C], isign [V, C])`` triple) for
        an ``latent_h x latent_w`` latent; the engine builds the inverse permutations and rejects a table that is not a bijection.
        ``views=None`` drops them.  May synchronise the stream (table upload), unlike the sampling loop."""
        from . import views as _views
        s = self._stream()
        if views is None:
            self._call("lt_set_views", None, None, None, 0, 0, 0, s)
            self._views_key = None
            return
        if isinstance(views, tuple) and len(views) == 3 and all(isinstance(t, torch.Tensor) for t in views):
            perm, vsign, isign = views
        else:
            perm, vsign, isign = _views.stack_tables(list(views), latent_h, latent_w, self.in_channels)
        if perm.dim() != 2 or perm.shape[1] != latent_h * latent_w:
            raise LuminaLibError(f"set_views: view tables of shape {tuple(perm.shape)} do not match a {latent_h}x{latent_w} latent "
                                 f"([V, {latent_h * latent_w}] expected)")
        V = perm.shape[0]
        if tuple(vsign.shape) != (V, self.in_channels) or tuple(isign.shape) != (V, self.in_channels):
            raise LuminaLibError(f"set_views: signs must be [V = {V}, C = {self.in_channels}], got {tuple(vsign.shape)} / {tuple(isign.shape)}")
        perm_d = perm.to(device=self.device, dtype=torch.int32).contiguous()
        vs = vsign.detach().to("cpu", torch.float32).contiguous()
        isg = isign.detach().to("cpu", torch.float32).contiguous()
        self._views_key = None
        self._call("lt_set_views", self._dev(perm_d), self._host(vs), self._host(isg), V, int(latent_h), int(latent_w), s)
        self._views_key = (V, int(latent_h), int(latent_w))

    def sample_views(self, z: torch.Tensor, tgrid, method: str = "midpoint", *, cfg_scale: float = 1.0, scale_factor: float = 1.0,
                     scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                     return_trajectory: bool = True) -> torch.Tensor:
        """Phase Init of the reference's visual_anagrams/generate.py:389-414 in ONE call: ``z`` is one latent ``[1, C, H, W]``; every stage
        of every interval evaluates all V views as one ``forward_with_cfg`` of 2 V rows.  Needs ``set_views`` and a prompt prepared at
        B = 2 V (rows 0..V-1 the view prompts, rows V..2V-1 the negative prompt).  Returns ``[n_grid, C, H, W]`` (or the last latent
        ``[1, C, H, W]``)."""
        _require_gpu(z, "z")
        garr, n, code, _ = self._fixed_grid(method, tgrid)
        if z.dim() != 4 or z.shape[0] != 1:
            raise LuminaLibError(f"sample_views takes ONE latent [1, C, H, W], got {tuple(z.shape)}")
        key = getattr(self, "_views_key", None)
        if key is None:
            raise LuminaLibError("sample_views: no views uploaded (call set_views first)")
        z = z.contiguous()
        a = self._step_args(z, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn)
        a.batch = 2 * key[0]
        out, traj_ptr, fin_ptr = _traj_or_final(z, n, z.shape[1:], return_trajectory)
        self._call("lt_sample_views", self._dev(z), traj_ptr, fin_ptr, garr, n, code, C.byref(a), self._stream())
        return out

    def set_softmax_rule(self, rule) -> None:
        """which reference's proportional-attention softmax scale this engine evaluates from now on (``lt_set_softmax_rule``): ``"t2i"`` /
        ``LT_SOFTMAX_T2I`` (default) or ``"anagram"`` / ``LT_SOFTMAX_ANAGRAM``, the rule of visual_anagrams/models/nextdit.py:333"""
        code = _lib.SOFTMAX_RULES.get(rule, rule) if isinstance(rule, str) else rule
        if isinstance(code, str):
            raise LuminaLibError(f"softmax rule '{rule}' not in {sorted(_lib.SOFTMAX_RULES)}")
        self._call("lt_set_softmax_rule", int(code))
        self.softmax_rule = int(code)

    def sample_views_guided(self, z: torch.Tensor, guidance: torch.Tensor, tgrid, coef: torch.Tensor, *, noise: Optional[torch.Tensor] = None,
                            cfg_scale: float = 1.0, scale_factor: float = 1.0, scale_watershed: float = 0.0, base_seqlen: Optional[int] = None,
                            proportional_attn: bool = False, return_trajectory: bool = True) -> torch.Tensor:
        """Phase Upscale of the reference's visual_anagrams/generate.py:465-494 in ONE call (``lt_sample_views_guided``): ``z``, ``guidance`` and
        ``noise`` (default: ``z``) are ``[1, C, H, W]`` in one dtype; ``coef`` is the fp32 CPU table ``[len(tgrid) - 1, 2, 4]`` of
        ``transport.integrators.views_guided_table``.  Needs ``set_views`` and a prompt prepared at B = 2 V, as ``sample_views``; the softmax
        rule is whatever ``set_softmax_rule`` left on the engine.  Returns ``[n_grid, C, H, W]`` (or the last latent ``[1, C, H, W]``)."""
        _require_gpu(z, "z")
        _require_gpu(guidance, "guidance")
        noise = z if noise is None else noise
        _require_gpu(noise, "noise")
        if z.dim() != 4 or z.shape[0] != 1:
            raise LuminaLibError(f"sample_views_guided takes ONE latent [1, C, H, W], got {tuple(z.shape)}")
        for name, t in (("guidance", guidance), ("noise", noise)):
            if tuple(t.shape) != tuple(z.shape) or t.dtype != z.dtype or t.device != z.device:
                raise LuminaLibError(f"sample_views_guided: {name} must be {tuple(z.shape)} {z.dtype} on {z.device}, got {tuple(t.shape)} {t.dtype} "
                                     f"on {t.device}")
        key = getattr(self, "_views_key", None)
        if key is None:
            raise LuminaLibError("sample_views_guided: no views uploaded (call set_views first)")
        z, guidance, noise = z.contiguous(), guidance.contiguous(), noise.contiguous()
        garr, n = _grid_array(tgrid)
        coef = coef.detach().to("cpu", torch.float32).contiguous()
        if tuple(coef.shape) != (max(n - 1, 0), 2, 4):
            raise LuminaLibError(f"sample_views_guided: coef must be [{max(n - 1, 0)}, 2, 4] (intervals, stages, ft f1t kc k1c), got {tuple(coef.shape)}")
        a = self._step_args(z, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn)
        a.batch = 2 * key[0]
        out, traj_ptr, fin_ptr = _traj_or_final(z, n, z.shape[1:], return_trajectory)
        self._call("lt_sample_views_guided", self._dev(z), self._dev(guidance), self._dev(noise), traj_ptr, fin_ptr, garr, self._host(coef), n,
                   C.byref(a), self._stream())
        return out

    # ---- tiled (MultiDiffusion) sampling: one canvas, the model on overlapping windows of it ---------------------
    def set_windows(self, offsets, win_hw, canvas_hw, weights: Optional[torch.Tensor] = None) -> None:
        """upload a window table (lt_set_windows): ``offsets`` ``[(top, left), ...]`` in latent pixels (``transport.tiled.window_grid``), every
        window ``win_hw``, on a canvas ``canvas_hw``; ``weights`` fp32 ``[win_h, win_w]`` (``transport.tiled.window_weights``; ``None``: ones).
        The engine refuses, by name, a table it cannot serve or that leaves a pixel of the canvas uncovered.  ``offsets=None`` drops the
        table.  Synchronises the stream once (the cover check), unlike the sampling loop."""
        s = self._stream()
        if offsets is None:
            self._call("lt_set_windows", None, 0, 0, 0, 0, 0, None, s)
            self._windows_key = None
            return
        offs = [(int(t), int(l)) for t, l in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
        (h, w), (Hc, Wc) = (int(v) for v in win_hw), (int(v) for v in canvas_hw)
        wd = None
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (h, w):
                raise LuminaLibError(f"set_windows: weights must be a tensor [{h}, {w}] (transport.tiled.window_weights)")
            wd = weights.detach().to(device=self.device, dtype=torch.float32).contiguous()
        arr = (C.c_int32 * max(2 * len(offs), 1))(*[v for o in offs for v in o])
        self._call("lt_set_windows", arr, len(offs), h, w, Hc, Wc, self._dev(wd), s)  # (a refusal leaves the table in force, and its key)
        self._windows_key = (len(offs), h, w, Hc, Wc)

    def _tiled_args(self, y: torch.Tensor, what: str, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor):
        _require_gpu(y, "y")
        key = getattr(self, "_windows_key", None)
        if key is None:
            raise LuminaLibError(f"{what}: no window table (call set_windows first)")
        n, h, w, Hc, Wc = key
        if y.dim() != 4 or tuple(y.shape) != (1, self.in_channels, Hc, Wc):
            raise LuminaLibError(f"{what} takes ONE canvas latent [1, {self.in_channels}, {Hc}, {Wc}] (the window table's canvas), got "
                                 f"{tuple(y.shape)}")
        a = self._step_args(y, cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor=ntk_factor)
        a.batch, a.latent_h, a.latent_w = 2 * n, h, w
        return a

    def forward_tiled(self, y: torch.Tensor, t: torch.Tensor, *, cfg_scale: float = 1.0, scale_factor: float = 1.0, scale_watershed: float = 1.0,
                      base_seqlen: Optional[int] = None, proportional_attn: bool = False, ntk_factor: float = 1.0) -> torch.Tensor:
        """one canvas evaluation (lt_forward_tiled; ``transport.tiled.tiled_velocity`` is the definition): the n windows of ``y [1, C, Hc, Wc]``
        as one ``forward_with_cfg`` of 2 n rows at ``t`` (2 n stage times), their predictions fused.  Needs ``set_windows`` and a conditioning
        prepared at B = 2 n (rows 0 .. n-1 the window prompts, rows n .. 2n-1 the negative prompts)."""
        a = self._tiled_args(y, "forward_tiled", cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor)
        y, t32, out = self._eval_io(y, t, name="y")
        if t32.numel() != a.batch:
            raise LuminaLibError(f"forward_tiled: t has {t32.numel()} entries, the {a.batch // 2} windows are evaluated as {a.batch} rows")
        self._call("lt_forward_tiled", self._dev(y), self._dev(t32), self._dev(out), C.byref(a), self._stream())
        return out

    def sample_ode_tiled(self, z: torch.Tensor, tgrid, method: str = "midpoint", *, cfg_scale: float = 1.0, scale_factor: float = 1.0,
                         scale_watershed: float = 1.0, base_seqlen: Optional[int] = None, proportional_attn: bool = False,
                         t_round_to_state_dtype: bool = True, return_trajectory: bool = True, ntk_factor: float = 1.0) -> torch.Tensor:
        """the fixed-grid trajectory of ONE canvas latent ``z [1, C, Hc, Wc]`` in one call (lt_sample_ode_tiled;
        ``transport.tiled.sample_tiled`` is the definition): every stage is ``forward_tiled``, the steps are ``sample_ode``'s.  Returns
        ``[n_grid, 1, C, Hc, Wc]`` or the last canvas."""
        garr, n, code, _ = self._fixed_grid(
            method, tgrid, f"sample_ode_tiled: tiled sampling is built for the fixed-grid methods {sorted(_lib.ODE_METHODS)}, not '{method}' "
                           "(the multistep and adaptive solvers are not served)")
        a = self._tiled_args(z, "sample_ode_tiled", cfg_scale, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor)
        z = z.contiguous()
        out, traj_ptr, fin_ptr = _traj_or_final(z, max(n, 1), z.shape, return_trajectory)
        self._call("lt_sample_ode_tiled", self._dev(z), traj_ptr, fin_ptr, garr, n, code, int(t_round_to_state_dtype), C.byref(a),
                   self._stream())
        return out

    # ---- composed guidance: K weighted prompts and one base prompt per image --------------------------------------
    def _compose_args(self, x: torch.Tensor, K: int, what: str, scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor,
                      cfg_channels) -> LtStepArgs:
        _require_gpu(x, "x")
        if x.dim() != 4:
            raise LuminaLibError(f"{what} takes a state [B', C, H, W], got {tuple(x.shape)}")
        a = self._step_args(x, 1.0, scale_factor, scale_watershed, base_seqlen, proportional_attn, cfg_channels=int(cfg_channels),
                            ntk_factor=ntk_factor)
        a.batch = (K + 1) * x.shape[0]
        return a

    def forward_compose(self, x: torch.Tensor, t: torch.Tensor, weights, *, scale_factor: float = 1.0, scale_watershed: float = 1.0,
                        base_seqlen: Optional[int] = None, proportional_attn: bool = False, ntk_factor: float = 1.0,
                        cfg_channels: int = 3) -> torch.Tensor:
        """one composed evaluation (lt_forward_compose; ``transport.guidance.guided_compose`` around the plain forward is the definition): the
        state ``x [B', C, H, W]`` under the K prompts and the base prompt as ONE plain forward of ``(K + 1) B'`` rows at ``t`` (that many stage
        times), composed with the K ``weights``.  Needs the conditioning prepared for ``(K + 1) B'`` rows: prompt 1's, ..., prompt K's, the base."""
        from .transport.guidance import check_compose
        w = _refusing(check_compose, weights, rows=1, who="forward_compose")
        K = w.shape[1]
        a = self._compose_args(x, K, "forward_compose", scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor, cfg_channels)
        x, t32, out = self._eval_io(x, t)
        if t32.numel() != a.batch:
            raise LuminaLibError(f"forward_compose: t has {t32.numel()} entries, {x.shape[0]} image(s) under K = {K} prompts are evaluated as "
                                 f"{a.batch} rows")
        self._call("lt_forward_compose", self._dev(x), self._dev(t32), self._dev(out), self._host(w), K, C.byref(a), self._stream())
        return out

    def sample_ode_compose(self, z: torch.Tensor, tgrid, table, method: str = "midpoint", *, scale_factor: float = 1.0, scale_watershed: float = 1.0,
                           base_seqlen: Optional[int] = None, proportional_attn: bool = False, t_round_to_state_dtype: bool = True,
                           return_trajectory: bool = True, ntk_factor: float = 1.0, cfg_channels: int = 3) -> torch.Tensor:
        """the composed fixed-grid trajectory of ``z [B', C, H, W]`` in one call (lt_sample_ode_compose; ``transport.guidance.sample_cfg_compose``
        is the definition): every stage is ``forward_compose`` with its row of ``table [(len(tgrid) - 1) * stages, K]``
        (``transport.guidance.compose_table``), the steps are ``sample_ode``'s.  Returns ``[n_grid, B', C, H, W]`` or the last state."""
        from .transport.guidance import check_compose
        garr, n, code, ncalls = self._fixed_grid(
            method, tgrid, f"sample_ode_compose: composed guidance is built for the fixed-grid methods {sorted(_lib.ODE_METHODS)}, not '{method}' "
                           "(the multistep and adaptive solvers are not served)")
        w = _refusing(check_compose, table, rows=max(ncalls, 1), who="sample_ode_compose")
        K = w.shape[1]
        a = self._compose_args(z, K, "sample_ode_compose", scale_factor, scale_watershed, base_seqlen, proportional_attn, ntk_factor, cfg_channels)
        z = z.contiguous()
        out, traj_ptr, fin_ptr = _traj_or_final(z, max(n, 1), z.shape, return_trajectory)
        self._call("lt_sample_ode_compose", self._dev(z), traj_ptr, fin_ptr, garr, n, code, self._host(w), K, int(t_round_to_state_dtype),
                   C.byref(a), self._stream())
        return out

    def last_nfe(self) -> int:
        return int(self.lib.lt_last_nfe(self.handle))

    def last_eval_rows(self) -> int:
        """the rows the last sampler call's evaluations ran, summed (``last_nfe() * batch`` unless conditional-only stages ran half)"""
        return int(self.lib.lt_last_eval_rows(self.handle))

    def graph_replays(self) -> int:
        """model evaluations served by a captured HIP graph so far"""
        return int(self.lib.lt_graph_replays(self.handle))

    # ---- mixture-of-experts routing hooks (parity tests) ----------------------------------------------
    def moe_routing_record(self, on: bool = True) -> None:
        self._call("lt_moe_routing_record", 1 if on else 0)

    def moe_routing_read(self, rows: int):
        """experts the last forward picked: int32 array [n_layers, 2 (time, token branch), rows, 2]; -1 = branch not run"""
        import numpy as np
        out = np.empty((int(self.cfg.n_layers), 2, rows, 2), dtype=np.int32)
        self._call("lt_moe_routing_read", out.ctypes.data_as(C.POINTER(C.c_int32)), rows)
        return out

    def moe_routing_force(self, sel=None) -> None:
        """sel int32 [n_layers, 2, rows, 2] (ascending expert ids per row) replaces the top-2 choice of the following forwards;
        None ends it"""
        import numpy as np
        if sel is None:
            self._call("lt_moe_routing_force", None, 0)
            return
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        assert sel.ndim == 4 and sel.shape[0] == int(self.cfg.n_layers) and sel.shape[1] == 2 and sel.shape[3] == 2, sel.shape
        self._call("lt_moe_routing_force", sel.ctypes.data_as(C.POINTER(C.c_int32)), sel.shape[2])

    # ---- profiling hooks used by bench.py -----------------------------------------------------------
    def profile_enable(self, on) -> None:
        """False / 0: off; True: every kernel class; int: bit mask (1 GEMM, 2 attention, 4 other)"""
        self._call("lt_profile_enable_mask", 7 if on is True else int(on))

    def profile_set_budget(self, klass: int, max_event_launches: int) -> None:
        self._call("lt_profile_set_budget", klass, max_event_launches)

    def profile_set_window(self, klass: int, skip_launches: int, max_event_launches: int) -> None:
        self._call("lt_profile_set_window", klass, skip_launches, max_event_launches)

    def profile_reset(self) -> None:
        self._call("lt_profile_reset")

    def profile_read(self, klass: int) -> Tuple[float, int, float]:
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self._call("lt_profile_read", klass, C.byref(ms), C.byref(n), C.byref(fl))
        return ms.value, n.value, fl.value


def ffn_hidden_dim(dim: int, multiple_of: int, ffn_dim_multiplier: Optional[float]) -> int:
    """FeedForward hidden width rule of the reference (lumina_next_t2i/models/model.py:469-473)."""
    hidden = int(2 * (4 * dim) / 3)
    if ffn_dim_multiplier is not None:
        hidden = int(ffn_dim_multiplier * hidden)
    return multiple_of * ((hidden + multiple_of - 1) // multiple_of)


def softmax_scale(seqlen: int, head_dim: int, proportional_attn: bool, base_seqlen: Optional[int], rule: int = _lib.LT_SOFTMAX_T2I) -> float:
    """model.py:373-376; ``rule=LT_SOFTMAX_ANAGRAM``: visual_anagrams/models/nextdit.py:331-335"""
    if proportional_attn:
        if rule == _lib.LT_SOFTMAX_ANAGRAM:
            return math.log(seqlen, base_seqlen) / math.sqrt(head_dim)
        return math.sqrt(math.log(seqlen, base_seqlen) / head_dim)
    return math.sqrt(1 / head_dim)


def anagram_chunks_cover(seqlen: int, base_seqlen: int) -> bool:
    """visual_anagrams/models/nextdit.py:336-352: the fork walks the queries in ``int(seqlen / base_seqlen + 0.99)`` chunks of ``base_seqlen``
    rows; False where they end before the rows do (the engine refuses such a shape under LT_SOFTMAX_ANAGRAM)"""
    return int(seqlen / base_seqlen + 0.99) * base_seqlen >= seqlen
