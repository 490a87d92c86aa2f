"""Tiled (MultiDiffusion, Bar-Tal et al. 2023) sampling: one canvas latent, the model evaluated on overlapping windows of it.

A large image pays attention over all of its tokens, runs the model far from the resolution it was trained at, and has to fit the engine's
``max_tokens``.  MultiDiffusion keeps ONE canvas latent; at every stage the model is evaluated on overlapping windows of training size - each
with its own prompt if wanted -, the window predictions are averaged, with weights, where windows overlap, and the ODE step is taken on the
canvas::

    f[k]   = model(crop_k(y), t, prompt_k)                       # all n windows as ONE forward_with_cfg of 2 n rows
    v      = (sum_k place_k(weight * f[k])) / (sum_k place_k(weight))
    y_next = step(y, v)                                          # euler / midpoint / rk4 exactly as fixed_grid_odeint steps

``fuse`` below IS the arithmetic, in plain torch ops: it defines the feature, runs callables that are not engine-backed, and is what the engine
calls (``lt_forward_tiled`` / ``lt_sample_ode_tiled``: a gather and a reduce kernel around one model evaluation) are held to, bit for bit.
The reference has no such sampler; the limits are reference-held: one window that is the canvas, with weight one, is ``fixed_grid_odeint``,
and disjoint windows are the per-crop trajectories."""
from __future__ import annotations

import math

import torch as th

from .integrators import FIXED_GRID_METHODS, fixed_grid_odeint

MAX_WINDOWS = 64  # the engine's table (LT_WINDOWS_MAX)
WEIGHT_KINDS = ("uniform", "cosine")


def _axis_offsets(canvas: int, win: int, stride: int):
    out, o = [], 0
    while o + win < canvas:
        out.append(o)
        o += stride
    out.append(canvas - win)  # the last window is clamped onto the canvas: its stride may be shorter
    return out


def window_grid(canvas_h: int, canvas_w: int, win_h: int, win_w: int, stride_h: int, stride_w: int, patch_size: int = 2):
    """Row-major ``(top, left)`` offsets, in latent pixels, of the windows of ``win_h x win_w`` that cover a ``canvas_h x canvas_w`` canvas at
    strides ``stride_h, stride_w``: ``0, stride, 2 stride, ...`` per axis, the last one clamped to ``canvas - win``.  Sizes and strides are
    positive multiples of ``patch_size`` (so the offsets are), ``win <= canvas`` and ``stride <= win`` (no gaps)."""
    vals = dict(canvas_h=canvas_h, canvas_w=canvas_w, win_h=win_h, win_w=win_w, stride_h=stride_h, stride_w=stride_w, patch_size=patch_size)
    for name, v in vals.items():
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"window_grid: {name} = {v!r} is not a positive integer")
    for name, v in vals.items():
        if name != "patch_size" and v % patch_size:
            raise ValueError(f"window_grid: {name} = {v} is not a multiple of the patch size {patch_size}")
    if win_h > canvas_h or win_w > canvas_w:
        raise ValueError(f"window_grid: a window of {win_h}x{win_w} is larger than the canvas {canvas_h}x{canvas_w}")
    if stride_h > win_h or stride_w > win_w:
        raise ValueError(f"window_grid: a stride of ({stride_h}, {stride_w}) above the window {win_h}x{win_w} leaves gaps")
    return [(t, l) for t in _axis_offsets(canvas_h, win_h, stride_h) for l in _axis_offsets(canvas_w, win_w, stride_w)]


def window_weights(win_h: int, win_w: int, kind: str = "uniform"):
    """the fp32 ``[win_h, win_w]`` weight of a window's pixels: ``uniform`` - ones; ``cosine`` - the outer product of
    ``0.5 (1 - cos(2 pi (i + 0.5) / n))`` per axis (strictly positive, symmetric), computed in float64 and rounded once"""
    if kind not in WEIGHT_KINDS:
        raise ValueError(f"window_weights: kind '{kind}' not in {WEIGHT_KINDS}")
    if win_h < 1 or win_w < 1:
        raise ValueError(f"window_weights: a window of {win_h}x{win_w}")
    if kind == "uniform":
        return th.ones(win_h, win_w, dtype=th.float32)

    def axis(n):
        i = th.arange(n, dtype=th.float64)
        return 0.5 * (1.0 - th.cos(2.0 * math.pi * (i + 0.5) / n))

    return th.outer(axis(win_h), axis(win_w)).to(th.float32)


def check_windows(offsets, win_hw, canvas_hw, weight=None):
    """the window table as ``fuse`` and the engine take it: ``[(top, left), ...]`` of 1 .. 64 windows, every one inside the canvas; ``weight``
    (if given) an fp32 ``[win_h, win_w]`` tensor.  Returns the offsets as a list of int pairs."""
    offs = [(int(t), int(l)) for t, l in (offsets.tolist() if isinstance(offsets, th.Tensor) else offsets)]
    (h, w), (Hc, Wc) = win_hw, canvas_hw
    if not 1 <= len(offs) <= MAX_WINDOWS:
        raise ValueError(f"tiled sampling takes 1 .. {MAX_WINDOWS} windows, got {len(offs)}")
    if h < 1 or w < 1 or h > Hc or w > Wc:
        raise ValueError(f"a window of {h}x{w} does not fit the canvas {Hc}x{Wc}")
    for k, (t, l) in enumerate(offs):
        if t < 0 or l < 0 or t + h > Hc or l + w > Wc:
            raise ValueError(f"window {k} at ({t}, {l}) of size {h}x{w} lies outside the canvas {Hc}x{Wc}")
    if weight is not None and (not isinstance(weight, th.Tensor) or tuple(weight.shape) != (h, w) or weight.dtype != th.float32):
        raise ValueError(f"window weights must be an fp32 tensor [{h}, {w}] (window_weights)")
    return offs


def cover(offsets, weight, canvas_hw):
    """``wsum`` fp32 ``[Hc, Wc]``: the weights of the windows that hold a pixel, summed in window order from zero"""
    h, w = weight.shape
    wsum = th.zeros(canvas_hw, dtype=th.float32, device=weight.device)
    for t, l in offsets:
        wsum[t:t + h, l:l + w] = wsum[t:t + h, l:l + w] + weight
    return wsum


def fuse(f, offsets, weight, canvas_hw, dtype):
    """THE arithmetic of the feature.  ``f [n, C, h, w]`` (state dtype): the window predictions; ``weight`` fp32 ``[h, w]``.  An fp32 canvas of
    zeros takes ``acc[:, win_k] = acc[:, win_k] + weight * f[k].float()`` for k = 0 .. n-1 in that order - the product and the sum two
    separately rounded fp32 operations (no addcmul, no fma) -, ``wsum`` the same accumulation of ``weight`` alone, and the result is
    ``acc / wsum``: one fp32 division, rounded once to ``dtype``.  Returns ``[C, Hc, Wc]``."""
    n, C, h, w = f.shape
    weight = weight.to(f.device)
    acc = th.zeros((C,) + tuple(canvas_hw), dtype=th.float32, device=f.device)
    for k, (t, l) in enumerate(offsets):
        prod = weight * f[k].float()
        acc[:, t:t + h, l:l + w] = acc[:, t:t + h, l:l + w] + prod
    return (acc / cover(offsets, weight, canvas_hw)).to(dtype)


def crop(y, offsets, win_hw):
    """the n windows of ``y [1, C, Hc, Wc]`` as ``[n, C, h, w]``: exact copies"""
    h, w = win_hw
    return th.stack([y[0, :, t:t + h, l:l + w] for t, l in offsets])


def tiled_velocity(model_fn, y, t, offsets, win_hw, weight, /, **kw):  # (positional only: the class-conditional families name their labels y)
    """one canvas evaluation: the n windows of ``y [1, C, Hc, Wc]`` stacked twice into the 2 n rows ``forward_with_cfg`` expects, ONE evaluation
    ``model_fn(rows, t, **kw)`` (``t``: 2 n stage times; the conditioning in ``kw``: rows 0 .. n-1 the window prompts, rows n .. 2n-1 the
    negative prompts), rows 0 .. n-1 of its result fused.  Returns ``[1, C, Hc, Wc]``."""
    n = len(offsets)
    win = crop(y, offsets, win_hw)
    out = model_fn(th.cat([win, win]), t, **kw)
    return fuse(out[:n], offsets, weight, tuple(y.shape[2:]), y.dtype)[None]


def sample_tiled(model_fn, z, tgrid, offsets, win_hw, weight, method="euler", **kw):
    """The tiled trajectory on the host: all ``len(tgrid)`` canvas states ``[len(tgrid), 1, C, Hc, Wc]``.  The stepping is
    ``fixed_grid_odeint`` itself - the stage times, the dt handling and every rounding point of the fixed-grid host loop ``lt_sample_ode`` is
    pinned to - over ``tiled_velocity`` (the stage time, rounded to the state dtype, as an fp32 vector of 2 n entries)."""
    if method not in FIXED_GRID_METHODS:
        raise ValueError(f"tiled sampling is built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not '{method}'")
    if z.dim() != 4 or z.shape[0] != 1:
        raise ValueError(f"tiled sampling takes ONE canvas latent [1, C, Hc, Wc], got {tuple(z.shape)}")
    weight = window_weights(*win_hw) if weight is None else weight
    offs = check_windows(offsets, win_hw, tuple(z.shape[2:]), weight)
    t = tgrid if isinstance(tgrid, th.Tensor) else th.tensor(list(tgrid), dtype=th.float32)
    if len(t) < 2:
        raise ValueError("tiled sampling needs at least 2 grid points")
    device = z.device
    rows = 2 * len(offs)

    def _fn(tt, y):
        tvec = th.ones(rows).to(device) * tt
        return tiled_velocity(model_fn, y, tvec, offs, win_hw, weight, **kw)

    return fixed_grid_odeint(_fn, z, t.to(device), method=method)


# what the tiled call does not combine with, refused by name in the Python wrappers (the C entries take none of them)
def refuse_with_tiled(method, **others):
    """``others``: name -> value of the features a call was given beside ``windows``; any that is set is refused by name"""
    names = {"cfg_table": "a guidance table (cfg_table)", "rule": "a rescale / norm limit (cfg_rescale, cfg_norm_limit)",
             "cfg_reuse": "guidance reuse (cfg_reuse)", "slg": "skip-layer guidance (slg_table)", "pag": "perturbed-attention guidance (pag_table)",
             "project": "projected guidance (cfg_apg, cfg_zero_star)", "teacache": "step caching (teacache)", "mask": "an inpainting mask",
             "packed": "a packed batch (a list of latents)"}
    for key, v in others.items():
        if v is not None and v is not False:
            raise NotImplementedError(f"tiled sampling (windows) and {names.get(key, key)} are not served together")
    if method not in FIXED_GRID_METHODS:
        raise NotImplementedError(f"tiled sampling (windows) is built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not '{method}' "
                                  "(the multistep and adaptive solvers are not served)")


def sample_tiled_front(x, model, tgrid, method, model_kwargs, windows, weights, *, t_round=True, use_engine=True, **others):
    """``sample(..., windows=(offsets, (win_h, win_w)), window_weights=)`` of both ODE front ends: the refusals by name, then ONE
    ``lt_sample_ode_tiled`` call for an engine-backed ``forward_with_cfg`` on a ROCm state, the host loop ``sample_tiled`` for any other callable
    (whose conditioning then has its 2 n rows already).  ``others``: the features the call was given beside the windows."""
    from .integrators import _engine_target
    refuse_with_tiled(method, packed=True if isinstance(x, (list, tuple)) else None, **others)
    try:
        offsets, win_hw = windows
        win_hw = (int(win_hw[0]), int(win_hw[1]))
    except (TypeError, ValueError):
        raise ValueError("windows must be (offsets, (win_h, win_w)) - transport.tiled.window_grid builds the offsets") from None
    target = _engine_target(model)
    if target is not None and not target[1]:
        raise TypeError("tiled sampling evaluates the windows as forward_with_cfg rows (window prompts, then negative prompts): it needs the bound "
                        "forward_with_cfg, not forward")
    if target is not None and x.is_cuda and use_engine and hasattr(target[0], "_engine_sample_ode_tiled"):
        return target[0]._engine_sample_ode_tiled(x, tgrid, method, t_round, (offsets, win_hw), weights, dict(model_kwargs))
    return sample_tiled(model, x, tgrid, offsets, win_hw, weights, method, **model_kwargs)
