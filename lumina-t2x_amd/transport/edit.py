"""Prompt-driven image editing: FlowEdit's inversion-free rule (Kulikov et al., 2024) on Lumina's path.

Lumina's path is ``x_t = t x1 + (1 - t) x0`` (noise at t = 0, data at t = 1) and the grid ascends.  With a source latent ``x_src``, an edit state
``z`` (``x_src`` itself at the first grid point), one noise draw per interval and the conditioning of FOUR rows per image - source prompt,
target prompt and their two negative prompts - interval ``i`` is::

    t   = float(tgrid[i])                                   # an fp32 grid value; omt = 1 - t and dt = float(tgrid[i+1]) - t are doubles
    zs  = x_src * t + noise[i] * (1 - t)                    # the source on the straight path at t
    zt  = zs + (z - x_src)                                  # the edit, shifted by the same amount
    c_s, c_t, u_s, u_t = model_fn(cat([zs, zt, zs, zt]), full(4 B', t), <conditioning>)      # ONE plain forward of 4 B' rows
    v_s = u_s + w_s * (c_s - u_s),  v_t = u_t + w_t * (c_t - u_t)      on the channels < ch (forward_with_cfg's expression, per branch);
    v_s = c_s,  v_t = c_t                                              on the others
    z'  = z + (v_t - v_s) * dt

There is no inversion and one model evaluation per interval.  ``zt`` is ``zs + (z - x_src)`` and NOT the left-to-right ``(z + zs) - x_src``: the
edit delta ``z - x_src`` is small next to ``zs`` while the edit is young, and the sum ``z + zs`` would round it away in bf16; as written the delta
is exact, and ``z == x_src`` gives ``zt == zs`` bit for bit.  Every tensor op rounds to the state dtype on its own; the scalars are Python floats
that multiply in fp32.  Only euler is defined - the rule has no higher-order form.  Averaging the velocity difference over several noise draws per
interval (``n_avg`` in the paper) is out of scope.

``sample_flowedit`` below IS that text in plain torch ops: it defines the feature, runs any callable, and is what the engine call
(``lt_sample_flowedit``: the two chains as fused kernels around one graph-cached evaluation) is held to, state for state.  The reference has no
such sampler."""
from __future__ import annotations

import math

import torch as th

METHODS = ("euler",)
ROWS = 4  # rows of one evaluation per edited image: source, target, negative source, negative target


def _grid32(tgrid):
    """the fp32 grid's values on the host (what ``float(tgrid[i])`` reads)"""
    t = tgrid if isinstance(tgrid, th.Tensor) else th.tensor(list(tgrid), dtype=th.float32)
    return t.detach().to("cpu", th.float32)


def check_method(method):
    if method not in METHODS:
        raise NotImplementedError(f"FlowEdit is defined for the euler method only (the rule has no higher-order form), not '{method}'")


def flowedit_scales(n, src_cfg, tgt_cfg):
    """the ``[n, 2]`` fp32 table of ``(w_s, w_t)`` pairs of ``n`` intervals; each argument is one float for all intervals or a sequence of ``n``"""
    n = int(n)
    if n < 1:
        raise ValueError(f"FlowEdit needs at least one interval, got {n}")
    cols = []
    for name, v in (("src_cfg", src_cfg), ("tgt_cfg", tgt_cfg)):
        if isinstance(v, (int, float)):
            col = th.full((n,), float(v), dtype=th.float32)
        else:
            col = th.as_tensor(v).detach().to("cpu", th.float32).reshape(-1)
            if col.numel() != n:
                raise ValueError(f"{name} has {col.numel()} entries for {n} intervals (one float, or one per interval)")
        if not bool(th.isfinite(col).all()):
            raise ValueError(f"{name} has an entry that is not finite")
        cols.append(col)
    return th.stack(cols, 1).contiguous()


def check_scales(scales, n):
    """a ready ``[n, 2]`` table as fp32 on the host"""
    s = th.as_tensor(scales).detach().to("cpu", th.float32)
    if tuple(s.shape) != (n, 2):
        raise ValueError(f"FlowEdit scales must be [{n}, 2] (one (w_s, w_t) pair per interval), got {tuple(s.shape)}")
    if not bool(th.isfinite(s).all()):
        raise ValueError("FlowEdit scales have an entry that is not finite")
    return s.contiguous()


def check_edit_operands(x_src, z, noise, n_intervals):
    """the source ``[B', C, H, W]``, the edit state (``None``: the source itself) and the noise ``[n_intervals, B', C, H, W]``: one shape, one
    dtype (bf16 or fp32), one device.  Returns ``(x_src, z, noise)``."""
    if not isinstance(x_src, th.Tensor) or x_src.dim() != 4:
        raise ValueError("FlowEdit: x_src must be a [B', C, H, W] tensor")
    if x_src.dtype not in (th.bfloat16, th.float32):
        raise ValueError(f"FlowEdit: state dtype {x_src.dtype} unsupported (bf16 or fp32)")
    z = x_src if z is None else z
    if not isinstance(z, th.Tensor) or tuple(z.shape) != tuple(x_src.shape) or z.dtype != x_src.dtype or z.device != x_src.device:
        raise ValueError(f"FlowEdit: z must have the shape, dtype and device of x_src {tuple(x_src.shape)} {x_src.dtype} on {x_src.device}")
    want = (int(n_intervals),) + tuple(x_src.shape)
    if not isinstance(noise, th.Tensor) or tuple(noise.shape) != want or noise.dtype != x_src.dtype or noise.device != x_src.device:
        got = f"{tuple(noise.shape)} {noise.dtype} on {noise.device}" if isinstance(noise, th.Tensor) else type(noise).__name__
        raise ValueError(f"FlowEdit: noise must be {want} {x_src.dtype} on {x_src.device} (one draw per interval), got {got}")
    return x_src, z, noise


def check_cond_rows(cond_kw, Bp):
    """every conditioning tensor carries 4 B' rows: [src_*, tgt_*, neg_src_*, neg_tgt_*]"""
    for k, v in cond_kw.items():
        if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] != ROWS * Bp:
            raise ValueError(f"FlowEdit: conditioning '{k}' has {v.shape[0]} rows; {Bp} image(s) need 4 B' = {ROWS * Bp} rows (source, target, "
                             "negative source, negative target), a batch that is a multiple of 4")


def mix(x_src, z, noise_i, t: float):
    """``(zs, zt)``: the source on the path at the Python float ``t``, and the edit shifted by the same amount"""
    zs = x_src * t + noise_i * (1 - t)
    return zs, zs + (z - x_src)


def edit_tail_start(z, x_src, noise, t: float):
    """the target-branch latent ``zt`` at ``t``: where ordinary guided sampling of the target prompt takes over from the edit (``--n_min``)"""
    return mix(x_src, z, noise, t)[1]


def guided_pair(out, w_s: float, w_t: float, ch: int):
    """``(v_s, v_t)`` of one evaluation's 4 B' rows ``[c_s, c_t, u_s, u_t]``: forward_with_cfg's expression per branch on the channels < ch"""
    c_s, c_t, u_s, u_t = out.chunk(ROWS)
    g_s = u_s[:, :ch] + w_s * (c_s[:, :ch] - u_s[:, :ch])
    g_t = u_t[:, :ch] + w_t * (c_t[:, :ch] - u_t[:, :ch])
    return th.cat([g_s, c_s[:, ch:]], 1), th.cat([g_t, c_t[:, ch:]], 1)


def combine(z, out, w_s: float, w_t: float, dt: float, ch: int):
    v_s, v_t = guided_pair(out, w_s, w_t, ch)
    return z + (v_t - v_s) * dt


def sample_flowedit(model_fn, x_src, tgrid, noise, scales, *, z=None, cfg_channels=3, method="euler", velocities=None, **cond_kw):
    """The edit trajectory on the host: every state ``[len(tgrid), B', C, H, W]``, slot 0 = ``z``.  ``model_fn(x [4 B', C, H, W], t fp32 [4 B'],
    **cond_kw)`` is a plain forward; ``scales`` is the ``[len(tgrid) - 1, 2]`` table of ``flowedit_scales``.  ``velocities`` (a list) receives
    ``(v_s, v_t)`` of every interval."""
    check_method(method)
    grid = _grid32(tgrid)
    if len(grid) < 2:
        raise ValueError("FlowEdit needs at least 2 grid points")
    n = len(grid) - 1
    x_src, z, noise = check_edit_operands(x_src, z, noise, n)
    w = check_scales(scales, n).tolist()
    Bp, C = x_src.shape[0], x_src.shape[1]
    check_cond_rows(cond_kw, Bp)
    if not 1 <= int(cfg_channels):
        raise ValueError(f"FlowEdit: cfg_channels {cfg_channels} must be at least 1")
    ch = min(int(cfg_channels), C)
    if not all(math.isfinite(float(v)) for v in grid):
        raise ValueError("FlowEdit: the grid has a value that is not finite")
    out = th.empty((n + 1,) + tuple(x_src.shape), dtype=x_src.dtype, device=x_src.device)
    out[0] = z
    for i in range(n):
        t = float(grid[i])
        dt = float(grid[i + 1]) - float(grid[i])
        zs, zt = mix(x_src, z, noise[i], t)
        tvec = th.full((ROWS * Bp,), t, dtype=th.float32, device=x_src.device)
        o = model_fn(th.cat([zs, zt, zs, zt]), tvec, **cond_kw)
        if velocities is not None:
            velocities.append(guided_pair(o, w[i][0], w[i][1], ch))
        z = combine(z, o, w[i][0], w[i][1], dt, ch)
        out[i + 1] = z
    return out


def edit(model, x_src, tgrid, noise, cond, src_cfg, tgt_cfg, *, z=None, return_trajectory=False, **step_kw):
    """front end: ``model.sample_flowedit`` (one engine call for an engine-backed model on a ROCm device) or, for any other model with a plain
    ``forward(x, t, *cond)``, the host loop above.  ``cond``: the conditioning tensors of 4 B' rows in call order."""
    if hasattr(model, "sample_flowedit"):
        return model.sample_flowedit(x_src, tgrid, noise, *cond, src_cfg=src_cfg, tgt_cfg=tgt_cfg, z=z, return_trajectory=return_trajectory, **step_kw)
    if step_kw:
        raise TypeError(f"step flags {sorted(step_kw)} need an engine-backed model (a plain forward takes none)")
    scales = flowedit_scales(len(_grid32(tgrid)) - 1, src_cfg, tgt_cfg)
    states = sample_flowedit(lambda x, t: model.forward(x, t, *cond), x_src, tgrid, noise, scales, z=z)
    return states if return_trajectory else states[-1]
