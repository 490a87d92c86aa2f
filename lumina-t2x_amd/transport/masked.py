"""Inpainting: fixed-grid ODE sampling that regenerates the region a mask selects and keeps the rest of a source latent.

Lumina's path is ``x_t = t x1 + (1 - t) x0`` (noise at t = 0, data at t = 1).  With a source latent ``x1``, the noise ``x0`` the trajectory
started from and a mask ``m`` in [0, 1] (1 = generate, 0 = keep), after EVERY full step - the one that reaches t = 1 included - the state is
pulled onto the known path where the mask says keep::

    known(t) = noise * (1 - t) + x1 * t                  # the expression of sample_img2img.py, t a Python float
    y_{i+1}  = step(y_i, t_i -> t_{i+1})                 # euler / midpoint / rk4 exactly as fixed_grid_odeint steps
    y_{i+1}  = y_{i+1} * m + known(t_{i+1}) * (1 - m)

Stage-internal states (the midpoint half step, rk4 stages 2-4) are not blended; ``z`` is taken as it is (the driver builds ``known(t_0)``).
``sample_masked`` below IS that text in plain torch ops: it defines the feature, runs callables that are not engine-backed, and is what the
engine call (``lt_sample_ode_masked``: the blend fused into each step's last kernel) is held to, state for state.  The reference has no
inpainting sampler; the limits are reference-held: ``m = 1`` everywhere is ``fixed_grid_odeint``, ``m = 0`` everywhere is the img2img mix."""
from __future__ import annotations

import torch as th

from .integrators import FIXED_GRID_METHODS, fixed_grid_odeint
from .multistep import MASKED_REFUSAL, MULTISTEP_METHODS


def known(noise, x1, t: float):
    """the state of the straight path between ``noise`` and ``x1`` at the Python float ``t``"""
    return noise * (1 - t) + x1 * t


def blend(y, mask, noise, x1, t: float):
    return y * mask + known(noise, x1, t) * (1 - mask)


def _grid_floats(tgrid):
    """the fp32 grid's values as Python floats (what ``float(tgrid[i])`` gives on the fp32 tensor every sampler here holds)"""
    t = tgrid if isinstance(tgrid, th.Tensor) else th.tensor(list(tgrid), dtype=th.float32)
    return t.detach().to("cpu", th.float32)


def check_mask(mask):
    """a mask holds values in [0, 1] (outside it the blend extrapolates; NaN is refused too).  One host read."""
    if not isinstance(mask, th.Tensor) or not mask.is_floating_point():
        raise ValueError("inpainting mask must be a floating-point tensor with values in [0, 1] (1 = generate, 0 = keep)")
    if mask.numel() and not bool(((mask >= 0) & (mask <= 1)).all()):
        raise ValueError(f"inpainting mask has values outside [0, 1] (min {float(mask.min())}, max {float(mask.max())}): 1 = generate, 0 = keep")


def _expand_one(name, v, z):
    """``v`` broadcast to the state ``z``; a lower-rank operand gets leading axes first.  A batch of B / 2 is repeated for the second (uncond)
    half of a guidance batch."""
    if not isinstance(v, th.Tensor):
        raise ValueError(f"{name} must be a tensor that broadcasts to the state {tuple(z.shape)}")
    if v.dim() > z.dim():
        raise ValueError(f"{name} {tuple(v.shape)} has more axes than the state {tuple(z.shape)}")
    while v.dim() < z.dim():
        v = v[None]
    B = z.shape[0]
    if B % 2 == 0 and v.shape[0] * 2 == B and v.shape[0] != 1:
        v = v.repeat((2,) + (1,) * (z.dim() - 1))
    try:
        v = v.expand(z.shape)
    except RuntimeError:
        raise ValueError(f"{name} {tuple(v.shape)} does not broadcast to the state {tuple(z.shape)}") from None
    return v.to(device=z.device, dtype=z.dtype).contiguous()


def expand_operands(z, mask, x1, noise):
    """``mask`` ([H, W], [1|B, 1, H, W], ...), the source ``x1`` and the ``noise`` ([1|B', C, H, W], ...) in the layout and dtype of the state ``z
    [B, C, H, W]``: broadcast, an operand of B / 2 rows repeated for the uncond half of a guidance batch, and rounded to the state dtype - once,
    here.  The mask's values are checked (``check_mask``)."""
    check_mask(mask)
    return _expand_one("mask", mask, z), _expand_one("x1", x1, z), _expand_one("noise", noise, z)


def expand_operands_packed(zs, masks, x1s, noises):
    """the list form: sample b of each operand broadcasts to ``zs[b] [C, H_b, W_b]``; a list of len(zs) / 2 entries is repeated for the uncond half"""
    zs = list(zs)
    out = []
    for name, vs in (("mask", masks), ("x1", x1s), ("noise", noises)):
        vs = list(vs)
        if len(vs) * 2 == len(zs):
            vs = vs + vs
        if len(vs) != len(zs):
            raise ValueError(f"{name}: {len(vs)} entries for {len(zs)} samples (need one per sample, or one per sample of the first half)")
        if name == "mask":
            for v in vs:
                check_mask(v)
        out.append([_expand_one(f"{name}[{b}]", v, z) for b, (v, z) in enumerate(zip(vs, zs))])
    return out


def sample_masked(model_fn, z, tgrid, mask, x1, noise, method="euler", *, batch=None, **kw):
    """The masked trajectory on the host: every state ``[len(tgrid), *z.shape]``.  ``model_fn(y, tvec, **kw)`` is evaluated as the fixed-grid
    samplers evaluate it (``tvec`` an fp32 vector of ``batch`` entries, default ``z.size(0)``, holding the stage time rounded to the state
    dtype); each step is ``fixed_grid_odeint`` over one interval, then the blend at the interval's end.  ``mask``, ``x1`` and ``noise`` have the
    shape and dtype of ``z`` (``expand_operands``)."""
    if method in MULTISTEP_METHODS:
        raise NotImplementedError(MASKED_REFUSAL.format(method))
    if method not in FIXED_GRID_METHODS:
        raise ValueError(f"masked sampling is built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not '{method}'")
    for name, v in (("mask", mask), ("x1", x1), ("noise", noise)):
        if not isinstance(v, th.Tensor) or tuple(v.shape) != tuple(z.shape) or v.dtype != z.dtype:
            raise ValueError(f"{name} must have the shape and dtype of the state {tuple(z.shape)} {z.dtype} (expand_operands)")
    grid = _grid_floats(tgrid)
    if len(grid) < 2:
        raise ValueError("masked sampling needs at least 2 grid points")
    B = z.size(0) if batch is None else batch
    device = z.device
    t = grid.to(device)

    def _fn(tt, y):
        tvec = th.ones(B).to(device) * tt
        return model_fn(y, tvec, **kw)

    out = th.empty((len(grid),) + tuple(z.shape), dtype=z.dtype, device=device)
    out[0] = z
    y = z
    for i in range(len(grid) - 1):
        y = fixed_grid_odeint(_fn, y, t[i:i + 2], method=method)[1]
        y = blend(y, mask, noise, x1, float(grid[i + 1]))
        out[i + 1] = y
    return out
