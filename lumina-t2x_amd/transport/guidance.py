"""Guidance schedules: fixed-grid ODE sampling whose classifier-free-guidance scale changes from stage to stage, and whose stages at scale 1
evaluate the conditional rows alone.

The state has ``B = 2 B'`` rows, cond rows then uncond rows, as every guided sampler here has; its first half is the sample (the reference's
``samples[:1]``).  ``table`` holds one fp32 scale per model evaluation: stage ``k`` of interval ``i`` uses ``w = table[i * stages + k]``
(``stages`` = 1 euler, 2 midpoint, 4 rk4)::

    w != 1   slope = model.forward_with_cfg(x, t, <conditioning>, cfg_scale=w, ...)          # B rows
    w == 1   o = model.forward(x[:B'], t[:B'], <cond half of the conditioning>)               # B' rows: half the cost
             slope = cat([o, o])

At ``w = 1`` the guided expression ``unc + 1 * (cond - unc)`` is the conditional output, so a guidance INTERVAL (guidance for ``lo <= t < hi``
only) is a table that holds 1 outside the interval - ``cfg_table`` builds it - and a guidance SCHEDULE (ramp, cosine, any function of t) is any
other table.  Under the reference's ``cfg_channels = 3`` quirk (guidance on the first three latent channels, the rest passed through row by
row) channel 3 of the SECOND half of a ``w == 1`` stage holds the cond rows' output where ``forward_with_cfg(cfg_scale=1)`` would leave the
uncond rows' own; the first half, the sample, does not see the difference within that stage.  It is written down here, not worked around.

``sample_cfg_schedule`` below IS that text in plain torch ops, as ``transport/masked.py`` is for inpainting: it defines the feature, runs
models that are not engine-backed and CPU states, and is what the engine call (``lt_sample_ode_cfg_schedule``) is held to, state for state.
It restates the loop of ``fixed_grid_odeint`` - same stage times, same ``dt`` handling, same rounding points.  The engine evaluates the
conditional rows with the step arguments of the guided evaluation; an engine-backed model's plain ``forward`` reads its RoPE arguments off
the module instead (``NextDiT._plain_forward_args``), so the two agree where those select the same table - ``scale_factor`` 1, or the
families whose factors persist on the module.

Rescaled and norm-limited guidance multiplies the guided output of every stage whose scale is not 1 by one factor per sample:
``guided_rule`` is the rule, ``sample_cfg_rule`` the loop around it - ``sample_cfg_schedule`` with another ``func`` - and
``lt_sample_ode_cfg_rule`` / ``lt_forward_cfg_rule`` are held to them word for word.

Guidance reuse takes the difference ``cond - uncond`` of the guided channels on some guided stages and reuses it on the others,
which evaluate the cond rows alone: ``sample_cfg_reuse`` / ``sample_cfg_reuse_multistep`` are the definition ``lt_sample_ode_cfg_reuse`` /
``lt_sample_ode_multistep_cfg_reuse`` are held to, ``cfg_reuse_table`` builds the flag tables and ``check_reuse`` refuses what the engine refuses.

Skip-layer guidance adds ``s (cond - skip)``, ``skip`` the cond rows evaluated with a set of blocks left out: ``sample_cfg_slg`` is
the definition ``lt_sample_ode_cfg_slg`` is held to, ``slg_table`` builds the table of ``s`` and ``slg_combine`` is the chain of roundings.

Perturbed-attention guidance takes the third prediction with a set of blocks PERTURBED - their self-attention map replaced by the
identity, so every query's output is its own value row - and, if wanted, another set left out: ``sample_cfg_pag`` is the definition
``lt_sample_ode_cfg_pag`` is held to, ``pag_table`` builds the table, and the chain of roundings is ``slg_combine`` unchanged.

Projected guidance replaces the guided expression by one built on inner products of the two predictions - APG's
momentum / norm-clip / projection, CFG-Zero*'s rescaled unconditional row and zero-init: ``guided_project`` is the form, ``sample_cfg_project`` the
loop ``lt_sample_ode_cfg_project`` is held to, ``check_project`` / ``refuse_with_project`` refuse what the engine refuses.

Composed guidance (Composable Diffusion, Liu et al. 2022) puts K weighted prompts and one base prompt on one image,
``g = u + sum_k w_k (c_k - u)``: the state has ``B'`` rows - there is no second half to carry - and every stage is ONE plain ``forward`` of
``(K + 1) B'`` rows.  ``guided_compose`` is the chain of roundings, ``sample_cfg_compose`` the loop ``lt_sample_ode_compose`` is held to,
``compose_table`` builds the per-stage weights and ``check_compose`` / ``refuse_with_compose`` refuse what the engine refuses."""
from __future__ import annotations

import math

import torch as th

from .integrators import FIXED_GRID_METHODS, _call, fixed_grid_odeint
from .multistep import MULTISTEP_METHODS

_STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


def _check_method(method, multistep=False):
    if multistep and method in MULTISTEP_METHODS:  # one evaluation per interval, at t0 (transport/multistep.py)
        return 1
    if method not in FIXED_GRID_METHODS:
        raise ValueError(f"guidance schedules are built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not '{method}'")
    return _STAGES[method]


def _grid32(tgrid):
    t = tgrid if isinstance(tgrid, th.Tensor) else th.tensor(list(tgrid), dtype=th.float32)
    t = t.detach().to("cpu", th.float32)
    if t.dim() != 1 or len(t) < 2:
        raise ValueError("a guidance schedule needs a 1-D grid of at least 2 points")
    return t


def stage_times(tgrid, method, state_dtype=th.float32, t_round=True):
    """The fp32 stage times ``[(len(tgrid) - 1) * stages]`` the engine hands the model, in evaluation order: ``t0``, for midpoint ``t0 + 0.5 dt``,
    for rk4 ``t0 + dt * fp32(1/3)``, ``t0 + dt * fp32(2/3)`` and ``t1`` - fp32 arithmetic on the fp32 grid, as ``fixed_grid_odeint`` forms them
    on 0-dim tensors.  With a bf16 state and ``t_round`` each is rounded to bf16 (torchdiffeq casts the time to the state dtype)."""
    stages = _check_method(method, multistep=True)
    t = _grid32(tgrid)
    t0, t1 = t[:-1], t[1:]
    dt = t1 - t0
    if stages == 1:  # euler, and the multistep methods
        cols = [t0]
    elif method == "midpoint":
        cols = [t0, t0 + 0.5 * dt]
    else:
        # a Python float times an fp32 tensor multiplies by the fp32 rounding of the float
        cols = [t0, t0 + dt * (1.0 / 3.0), t0 + dt * (2.0 / 3.0), t1]
    out = th.stack(cols, dim=1).reshape(-1)
    assert out.numel() == (len(t) - 1) * stages
    if t_round and state_dtype == th.bfloat16:
        out = out.to(th.bfloat16).to(th.float32)
    return out.contiguous()


def linear_schedule(cfg_scale, t0=0.0, t1=1.0):
    """``w(t)`` falling linearly from ``cfg_scale`` at ``t0`` (noise) to 1 at ``t1`` (data)"""
    return lambda t: cfg_scale + (1.0 - cfg_scale) * min(max((t - t0) / (t1 - t0), 0.0), 1.0)


def cosine_schedule(cfg_scale, t0=0.0, t1=1.0):
    """``w(t)`` falling from ``cfg_scale`` at ``t0`` to 1 at ``t1`` along half a cosine"""
    return lambda t: 1.0 + (cfg_scale - 1.0) * 0.5 * (1.0 + math.cos(math.pi * min(max((t - t0) / (t1 - t0), 0.0), 1.0)))


def cfg_table(tgrid, method, cfg_scale, interval=None, schedule=None):
    """The fp32 scale table of a trajectory.  ``interval=(lo, hi)``: ``cfg_scale`` where ``lo <= t_stage < hi``, 1 elsewhere; ``schedule``: a
    callable ``w(t)`` of the stage time as a Python float (inside the interval, when both are given); neither: ``cfg_scale`` everywhere.
    ``t_stage`` is the UNROUNDED fp32 stage time, so a table does not depend on the state dtype."""
    ts = stage_times(tgrid, method, th.float32, False).tolist()
    lo, hi = (-math.inf, math.inf) if interval is None else (float(interval[0]), float(interval[1]))
    if not lo <= hi:
        raise ValueError(f"guidance interval [{lo}, {hi}) is empty or not ordered")
    vals = []
    for t in ts:
        w = 1.0
        if lo <= t < hi:
            w = float(schedule(t)) if schedule is not None else float(cfg_scale)
        vals.append(w)
    table = th.tensor(vals, dtype=th.float32)
    if not bool(th.isfinite(table).all()):
        raise ValueError("guidance table has an entry that is not finite")
    return table


def check_table(table, tgrid, method):
    """``table`` as an fp32 CPU tensor of ``(len(tgrid) - 1) * stages`` finite entries"""
    stages = _check_method(method, multistep=True)
    n = len(_grid32(tgrid))
    t = table if isinstance(table, th.Tensor) else th.tensor(list(table), dtype=th.float32)
    t = t.detach().to("cpu", th.float32).reshape(-1).contiguous()
    if t.numel() != (n - 1) * stages:
        raise ValueError(f"guidance table has {t.numel()} entries, a {n}-point {method} grid has {(n - 1) * stages} stages")
    if not bool(th.isfinite(t).all()):
        raise ValueError("guidance table has an entry that is not finite")
    return t


def _cond_half(v, B):
    """the cond half of one conditioning argument: tensors with a leading axis of B rows are cut, everything else passes"""
    if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] == B:
        return v[: B // 2]
    return v


def sample_cfg_schedule(model, z, tgrid, table, method="euler", *, cond=None, t_round=True, **kw):
    """The scheduled trajectory on the host: every state ``[len(tgrid), *z.shape]``.

    ``model`` has ``forward_with_cfg(x, t, **cond, cfg_scale=w, **kw)`` and ``forward(x, t, **cond)``.  ``cond`` names the conditioning kwargs
    (default: every tensor in ``kw`` whose leading axis has ``z.size(0)`` rows); the rest of ``kw`` goes to ``forward_with_cfg`` alone, as the
    reference's plain ``forward`` takes no such arguments.  ``t`` is the fp32 ``[B]`` vector of the fixed-grid samplers, holding the stage time
    rounded to the state dtype (``t_round``)."""
    stages = _check_method(method)
    table = check_table(table, tgrid, method)
    B = z.size(0)
    if B % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {B}")
    kw = dict(kw)
    kw.pop("cfg_scale", None)  # the table is the scale
    if cond is None:
        cond = [k for k, v in kw.items() if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] == B]
    cond_kw = {k: kw.pop(k) for k in cond}
    half_kw = {k: _cond_half(v, B) for k, v in cond_kw.items()}
    device = z.device
    t = _grid32(tgrid).to(device)
    w = table.tolist()
    call = [0]

    def func(tt, y):
        scale = w[call[0]]
        call[0] += 1
        tvec = th.ones(B).to(device) * tt  # fp32 [B] (reference integrators.py:108)
        if scale != 1.0:
            return model.forward_with_cfg(y, tvec, **cond_kw, cfg_scale=scale, **kw)
        o = model.forward(y[: B // 2], tvec[: B // 2], **half_kw)
        return th.cat([o, o])

    def f(tt, y):
        return _call(func, tt, y) if t_round else func(tt, y)

    # fixed_grid_odeint's loop (integrators.py), statement for statement
    out = th.empty((len(t),) + tuple(z.shape), dtype=z.dtype, device=device)
    out[0] = z
    y = z
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    for j in range(len(t) - 1):
        t0, t1 = t[j], t[j + 1]
        dt = t1 - t0
        k1 = f(t0, y)
        if method == "euler":
            dy = dt * k1
        elif method == "midpoint":
            half = 0.5 * dt
            dy = dt * f(t0 + half, y + k1 * half)
        else:
            k2 = f(t0 + dt * third, y + dt * k1 * third)
            k3 = f(t0 + dt * two_thirds, y + dt * (k2 - k1 * third))
            k4 = f(t1, y + dt * (k1 - k2 + k3))
            dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        y = y + dy
        out[j + 1] = y
    assert call[0] == (len(t) - 1) * stages
    return out


# ---- rescaled and norm-limited guidance ---------------------------------------------------------------------------------------
def check_rule(rescale, norm_limit):
    """``(rescale, norm_limit)`` as the fp32 values the engine reads, as Python floats; refuses a blend outside [0, 1] and a limit that is not
    above 0 (``inf``: no limit)"""
    rescale, norm_limit = float(rescale), float(norm_limit)
    if not (math.isfinite(rescale) and 0.0 <= rescale <= 1.0):
        raise ValueError(f"guidance rescale {rescale} is not a blend in [0, 1]")
    if math.isnan(norm_limit) or not norm_limit > 0.0:
        raise ValueError(f"guidance norm_limit {norm_limit} is not above 0 (inf switches the limit off)")
    return float(th.tensor(rescale, dtype=th.float32)), float(th.tensor(norm_limit, dtype=th.float32))


def rule_is_off(rescale, norm_limit):
    """the defaults: no rescale, no limit - callers then make the call they made before the rule existed"""
    return float(rescale) == 0.0 and float(norm_limit) == math.inf


def rule_factor(Sc, Scc, Sg, Sgg, n, rescale, norm_limit):
    """``(f, fr, fl)`` of one sample from its four float64 sums: float64 arithmetic operation by operation (Python floats: no fused
    multiply-add), ``f`` rounded once to fp32"""
    mc, mg = Sc / n, Sg / n
    vc = Scc / n - mc * mc
    vg = Sgg / n - mg * mg
    ratio = math.sqrt(vc / vg) if (vg > 0.0 and vc >= 0.0) else 1.0
    fr = rescale * ratio + (1.0 - rescale)
    fl = 1.0
    den = fr * math.sqrt(Sgg)
    if norm_limit < math.inf and den > 0.0:
        fl = min(1.0, norm_limit * math.sqrt(Scc) / den)
    return float(th.tensor(fr * fl, dtype=th.float64).to(th.float32)), fr, fl


def guided_rule(o, w, ch, rescale=0.0, norm_limit=math.inf, parts=None):
    """The rule at scale ``w`` on a model output ``o [B, C, H, W]`` (cond rows, then uncond rows; taken as bf16, returned in its own dtype): ``(out, f)``.

    ``g = u + w (c - u)`` on the first ``ch`` channels in bf16 tensor ops (every op rounds: the closing kernel's chain); per sample the float64
    sums of ``c``, ``c^2``, ``g``, ``g^2``; ``f = fp32(fr * fl)`` with ``fr = rescale * sqrt(var c / var g) + (1 - rescale)`` and ``fl = min(1,
    norm_limit * |c| / (fr * |g|))`` (``rule_factor``); ``gg = bf16(fp32(g) * f)``; the channels past ``ch`` pass through row by row.  ``fr``
    is the single-factor form of the published ``phi * g * ratio + (1 - phi) * g``, and the limit acts on ``fr * |g|``, the norm before the
    last rounding, so one reduction serves both.  ``rescale`` / ``norm_limit`` are taken as fp32 values.  ``f``: fp32 ``[B / 2]`` on ``o``'s
    device.  ``parts`` (a list): receives ``(fr, fl)`` per sample."""
    rescale, norm_limit = check_rule(rescale, norm_limit)
    B = o.size(0)
    if B % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {B}")
    half = B // 2
    ch = min(int(ch), o.size(1))
    dtype = o.dtype
    o = o.to(th.bfloat16)  # the model's output is bf16 (an engine-backed model hands an fp32 state the same values in fp32)
    c, u = o[:half, :ch], o[half:, :ch]
    g = u + w * (c - u)
    n = float(ch * o.size(2) * o.size(3))
    cd, gd = c.double().reshape(half, -1), g.double().reshape(half, -1)
    sums = th.stack([cd.sum(1), (cd * cd).sum(1), gd.sum(1), (gd * gd).sum(1)], dim=1).tolist()
    fs = []
    for Sc, Scc, Sg, Sgg in sums:
        f, fr, fl = rule_factor(Sc, Scc, Sg, Sgg, n, rescale, norm_limit)
        fs.append(f)
        if parts is not None:
            parts.append((fr, fl))
    f = th.tensor(fs, dtype=th.float32, device=o.device)
    gg = (g.float() * f.view(-1, 1, 1, 1)).to(th.bfloat16)
    out = th.cat([th.cat([gg, o[:half, ch:]], 1), th.cat([gg, o[half:, ch:]], 1)])
    return out.to(dtype), f


def sample_cfg_rule(model, z, tgrid, table, method="euler", *, rescale=0.0, norm_limit=math.inf, cond=None, t_round=True, factors=None, parts=None, **kw):
    """``sample_cfg_schedule`` whose stages at a scale other than 1 run ``guided_rule`` on ``model.forward`` of all ``B`` rows (both halves of
    the input are the first half, as ``forward_with_cfg`` makes them); a stage at scale 1 exactly is the conditional-only stage, without the
    rule.  ``model.cfg_channels`` (default 3) names the guided channels.  ``factors`` (a list): receives the fp32 ``[B / 2]`` factors of every
    guided stage, in evaluation order, ``parts`` (a list) their ``(fr, fl)`` per sample.  Stage times, table handling and the loop are ``sample_cfg_schedule``'s, statement for statement."""
    stages = _check_method(method)
    table = check_table(table, tgrid, method)
    rescale, norm_limit = check_rule(rescale, norm_limit)
    B = z.size(0)
    if B % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {B}")
    kw = dict(kw)
    kw.pop("cfg_scale", None)  # the table is the scale
    if cond is None:
        cond = [k for k, v in kw.items() if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] == B]
    cond_kw = {k: kw.pop(k) for k in cond}
    half_kw = {k: _cond_half(v, B) for k, v in cond_kw.items()}
    ch = int(getattr(model, "cfg_channels", 3))
    device = z.device
    t = _grid32(tgrid).to(device)
    w = table.tolist()
    call = [0]

    def func(tt, y):
        scale = w[call[0]]
        call[0] += 1
        tvec = th.ones(B).to(device) * tt  # fp32 [B] (reference integrators.py:108)
        if scale != 1.0:
            o = model.forward(th.cat([y[: B // 2]] * 2), tvec, **cond_kw)
            out, f = guided_rule(o, scale, ch, rescale, norm_limit, parts)
            if factors is not None:
                factors.append(f)
            return out.to(y.dtype)
        o = model.forward(y[: B // 2], tvec[: B // 2], **half_kw)
        return th.cat([o, o])

    def f(tt, y):
        return _call(func, tt, y) if t_round else func(tt, y)

    # fixed_grid_odeint's loop (integrators.py), statement for statement
    out = th.empty((len(t),) + tuple(z.shape), dtype=z.dtype, device=device)
    out[0] = z
    y = z
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    for j in range(len(t) - 1):
        t0, t1 = t[j], t[j + 1]
        dt = t1 - t0
        k1 = f(t0, y)
        if method == "euler":
            dy = dt * k1
        elif method == "midpoint":
            half = 0.5 * dt
            dy = dt * f(t0 + half, y + k1 * half)
        else:
            k2 = f(t0 + dt * third, y + dt * k1 * third)
            k3 = f(t0 + dt * two_thirds, y + dt * (k2 - k1 * third))
            k4 = f(t1, y + dt * (k1 - k2 + k3))
            dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        y = y + dy
        out[j + 1] = y
    assert call[0] == (len(t) - 1) * stages
    return out


# ---- a scale per evaluation of a multistep method -------------------------------------------------------------------------------
def sample_cfg_multistep(model, z, tgrid, table, method="abm2", *, rescale=0.0, norm_limit=math.inf, cond=None, t_round=True, factors=None,
                         parts=None, **kw):
    """``transport.multistep.multistep_odeint`` whose evaluation ``i`` is guided at ``table[i]`` (``len(tgrid) - 1`` entries): the evaluation of
    ``sample_cfg_schedule`` at the defaults, of ``sample_cfg_rule`` under a rescale blend or a norm limit - ``guided_rule`` per guided
    evaluation, the conditional rows alone at scale 1 exactly.  What ``lt_sample_ode_multistep`` with a table is held to, state for state."""
    from .multistep import multistep_odeint
    if method not in MULTISTEP_METHODS:
        raise ValueError(f"unknown multistep method '{method}' (built: {', '.join(MULTISTEP_METHODS)})")
    table = check_table(table, tgrid, method)
    rule_off = rule_is_off(rescale, norm_limit)
    rescale, norm_limit = check_rule(rescale, norm_limit)
    B = z.size(0)
    if B % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {B}")
    kw = dict(kw)
    kw.pop("cfg_scale", None)  # the table is the scale
    if cond is None:
        cond = [k for k, v in kw.items() if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] == B]
    cond_kw = {k: kw.pop(k) for k in cond}
    half_kw = {k: _cond_half(v, B) for k, v in cond_kw.items()}
    ch = int(getattr(model, "cfg_channels", 3))
    device = z.device
    w = table.tolist()
    call = [0]

    def func(tt, y):
        scale = w[call[0]]
        call[0] += 1
        tvec = th.ones(B).to(device) * tt  # fp32 [B] (reference integrators.py:108)
        if scale == 1.0:
            o = model.forward(y[: B // 2], tvec[: B // 2], **half_kw)
            return th.cat([o, o])
        if rule_off:
            return model.forward_with_cfg(y, tvec, **cond_kw, cfg_scale=scale, **kw)
        o = model.forward(th.cat([y[: B // 2]] * 2), tvec, **cond_kw)
        out, f = guided_rule(o, scale, ch, rescale, norm_limit, parts)
        if factors is not None:
            factors.append(f)
        return out.to(y.dtype)

    out = multistep_odeint(func, z, _grid32(tgrid), method, t_round=t_round)
    assert call[0] == len(w)
    return out


# ---- guidance reuse: the cond - uncond difference taken on refresh stages, reused in between -----------------------------------
def check_reuse(reuse, table, tgrid, method):
    """``(table, flags)``: the scale table of ``check_table`` and the reuse table as a list of 0 / 1, one per evaluation.  Refused: a wrong
    length, a flag other than 0 / 1, and - among the evaluations whose scale is not 1 - a reuse before the first refresh (at scale 1 exactly
    the evaluation is conditional-only under either flag)."""
    table = check_table(table, tgrid, method)
    r = reuse if isinstance(reuse, th.Tensor) else th.tensor(list(reuse))
    r = r.detach().to("cpu").reshape(-1)
    if r.numel() != table.numel():
        raise ValueError(f"reuse table has {r.numel()} entries, the guidance table has {table.numel()}")
    flags = []
    for i, v in enumerate(r.tolist()):
        if v not in (0, 1):  # (True / False included)
            raise ValueError(f"reuse flag {v} of evaluation {i} is not 0 (refresh) or 1 (reuse)")
        flags.append(int(v))
    stored = False
    for i, (w, f) in enumerate(zip(table.tolist(), flags)):
        if w == 1.0:
            continue
        stored = stored or f == 0
        if not stored:
            raise ValueError(f"evaluation {i} reuses the cond - uncond difference, but no refresh evaluation (flag 0 at a scale other than 1) "
                             "comes before it")
    return table, flags


def cfg_reuse_table(tgrid, method, table, every=2, interval=None, per_step=False):
    """The int32 flag table of a trajectory.  Among the evaluations with ``table != 1`` whose UNROUNDED stage time lies in ``interval = (lo, hi)``
    (``lo <= t < hi``; default: all of them) evaluation number ``j`` is a refresh (0) when ``j % every == 0``, else a reuse (1);
    ``per_step``: the first such evaluation of each grid interval is the refresh, its other stages reuse.  Entries at scale 1 are 0, guided
    entries outside the interval are refreshes, and the first guided evaluation of the trajectory is always a refresh."""
    stages = _check_method(method, multistep=True)
    table = check_table(table, tgrid, method)
    every = int(every)
    if every < 1:
        raise ValueError(f"cfg_reuse_table: every = {every} (1: refresh every guided evaluation)")
    lo, hi = (-math.inf, math.inf) if interval is None else (float(interval[0]), float(interval[1]))
    if not lo <= hi:
        raise ValueError(f"reuse interval [{lo}, {hi}) is empty or not ordered")
    ts = stage_times(tgrid, method, th.float32, False).tolist()
    flags, j, stored, last_step = [], 0, False, -1
    for i, (w, t) in enumerate(zip(table.tolist(), ts)):
        flag = 0
        if w != 1.0 and lo <= t < hi:
            if per_step:
                flag = 0 if i // stages != last_step else 1
                last_step = i // stages
            else:
                flag = 0 if j % every == 0 else 1
            j += 1
        if w != 1.0:
            if not stored:
                flag = 0
            stored = True
        flags.append(flag)
    return th.tensor(flags, dtype=th.int32)


def refuse_rule_with_reuse(rescale, norm_limit):
    """a reuse table together with a rescale blend or a norm limit is not served: the rule's sums need both halves of every guided stage"""
    if not rule_is_off(rescale, norm_limit):
        raise ValueError("guidance reuse (a reuse table) together with a rescale / norm_limit rule is not served: the rule's sums need the "
                         "cond and the uncond rows of every guided stage")


def _reuse_func(model, B, w, flags, cond_kw, half_kw, device, deltas=None):
    """the evaluation of ``sample_cfg_reuse`` / ``sample_cfg_reuse_multistep`` and its call counter"""
    ch_model = int(getattr(model, "cfg_channels", 3))
    call = [0]
    held = [None]  # d of the last refresh evaluation, bf16 [B', ch, H, W]

    def func(tt, y):
        scale, again = w[call[0]], flags[call[0]]
        call[0] += 1
        half = B // 2
        tvec = th.ones(B).to(device) * tt  # fp32 [B] (reference integrators.py:108)
        if scale == 1.0:  # the conditional-only stage of sample_cfg_schedule; d is neither read nor written
            o = model.forward(y[:half], tvec[:half], **half_kw)
            return th.cat([o, o])
        if not again:
            o = model.forward(th.cat([y[:half]] * 2), tvec, **cond_kw).to(th.bfloat16)  # (taken as bf16, as guided_rule takes it)
            ch = min(ch_model, o.size(1))
            c, u = o[:half, :ch], o[half:, :ch]
            d = c - u
            g = u + scale * d
            held[0] = d
            if deltas is not None:
                deltas.append(d)
            return th.cat([th.cat([g, o[:half, ch:]], 1), th.cat([g, o[half:, ch:]], 1)]).to(y.dtype)
        o = model.forward(y[:half], tvec[:half], **half_kw).to(th.bfloat16)
        d = held[0]
        ch = d.size(1)
        g = (o[:, :ch] - d) + scale * d
        r = th.cat([g, o[:, ch:]], 1)
        return th.cat([r, r]).to(y.dtype)

    return func, call


def _reuse_setup(z, kw, cond):
    B = z.size(0)
    if B % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {B}")
    kw = dict(kw)
    kw.pop("cfg_scale", None)  # the table is the scale
    refuse_rule_with_reuse(kw.pop("rescale", 0.0), kw.pop("norm_limit", math.inf))
    if cond is None:
        cond = [k for k, v in kw.items() if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] == B]
    cond_kw = {k: kw.pop(k) for k in cond}
    half_kw = {k: _cond_half(v, B) for k, v in cond_kw.items()}
    return B, cond_kw, half_kw


def sample_cfg_reuse(model, z, tgrid, table, reuse, method="euler", *, cond=None, t_round=True, deltas=None, **kw):
    """The trajectory of guidance reuse on the host: every state ``[len(tgrid), *z.shape]``.  This IS the definition ``lt_sample_ode_cfg_reuse``
    is held to, state for state.  Per evaluation ``table`` gives the scale ``w`` and ``reuse`` a flag:

        w == 1            o = model.forward(x[:B'], t[:B'], <cond half>);  slope = cat([o, o])                     # sample_cfg_schedule's
        w != 1, flag 0    o = bf16(model.forward(cat([x[:B']] * 2), t, <conditioning>));  d = c - u;  g = u + w * d   # B rows; d is kept
        w != 1, flag 1    o = bf16(model.forward(x[:B'], t[:B'], <cond half>));  g = (o - d) + w * d                  # B' rows; d is read

    on the first ``min(model.cfg_channels, C)`` channels in bf16 tensor ops (every op rounds), the other channels passing through row by row
    (refresh) or from the cond rows (reuse), ``g`` written to both halves, the result cast to the state dtype.  The loop is
    ``fixed_grid_odeint``'s, statement for statement.  ``deltas`` (a list): receives ``d`` of every refresh stage."""
    if isinstance(z, (list, tuple)):
        raise ValueError("guidance reuse takes a tensor state; a packed batch (a list of latents) is not served")
    stages = _check_method(method)
    table, flags = check_reuse(reuse, table, tgrid, method)
    B, cond_kw, half_kw = _reuse_setup(z, kw, cond)
    device = z.device
    t = _grid32(tgrid).to(device)
    func, call = _reuse_func(model, B, table.tolist(), flags, cond_kw, half_kw, device, deltas)

    def f(tt, y):
        return _call(func, tt, y) if t_round else func(tt, y)

    # fixed_grid_odeint's loop (integrators.py), statement for statement
    out = th.empty((len(t),) + tuple(z.shape), dtype=z.dtype, device=device)
    out[0] = z
    y = z
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    for j in range(len(t) - 1):
        t0, t1 = t[j], t[j + 1]
        dt = t1 - t0
        k1 = f(t0, y)
        if method == "euler":
            dy = dt * k1
        elif method == "midpoint":
            half = 0.5 * dt
            dy = dt * f(t0 + half, y + k1 * half)
        else:
            k2 = f(t0 + dt * third, y + dt * k1 * third)
            k3 = f(t0 + dt * two_thirds, y + dt * (k2 - k1 * third))
            k4 = f(t1, y + dt * (k1 - k2 + k3))
            dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        y = y + dy
        out[j + 1] = y
    assert call[0] == (len(t) - 1) * stages
    return out


def sample_cfg_reuse_multistep(model, z, tgrid, table, reuse, method="abm2", *, cond=None, t_round=True, deltas=None, **kw):
    """``transport.multistep.multistep_odeint`` around the evaluation of ``sample_cfg_reuse`` (``len(tgrid) - 1`` scales and flags): what
    ``lt_sample_ode_multistep_cfg_reuse`` is held to, state for state."""
    from .multistep import multistep_odeint
    if isinstance(z, (list, tuple)):
        raise ValueError("guidance reuse takes a tensor state; a packed batch (a list of latents) is not served")
    if method not in MULTISTEP_METHODS:
        raise ValueError(f"unknown multistep method '{method}' (built: {', '.join(MULTISTEP_METHODS)})")
    table, flags = check_reuse(reuse, table, tgrid, method)
    B, cond_kw, half_kw = _reuse_setup(z, kw, cond)
    func, call = _reuse_func(model, B, table.tolist(), flags, cond_kw, half_kw, z.device, deltas)
    out = multistep_odeint(func, z, _grid32(tgrid), method, t_round=t_round)
    assert call[0] == len(flags)
    return out


# ---- skip-layer guidance: a third prediction with a set of blocks left out, pushed away from -----------------------------------
def slg_table(tgrid, method, slg_scale, interval=None, what="skip-layer"):
    """The fp32 table of skip-layer scales of a trajectory, one per evaluation: ``slg_scale`` where ``lo <= t_stage < hi`` for
    ``interval = (lo, hi)`` (default: everywhere), 0 elsewhere.  ``t_stage`` is the UNROUNDED fp32 stage time, as in ``cfg_table``; an empty
    interval (``lo == hi``) gives all zeros."""
    ts = stage_times(tgrid, method, th.float32, False).tolist()
    lo, hi = (-math.inf, math.inf) if interval is None else (float(interval[0]), float(interval[1]))
    if not lo <= hi:
        raise ValueError(f"{what} interval [{lo}, {hi}) is not ordered")
    table = th.tensor([float(slg_scale) if lo <= t < hi else 0.0 for t in ts], dtype=th.float32)
    if not bool(th.isfinite(table).all()):
        raise ValueError(f"{what} table has an entry that is not finite")
    return table


def check_slg(slg, tgrid, method, what="skip-layer"):
    """``slg`` as an fp32 CPU tensor of ``(len(tgrid) - 1) * stages`` finite entries"""
    stages = _check_method(method)
    n = len(_grid32(tgrid))
    if slg is None:
        raise ValueError(f"{what} table is None (one scale per evaluation; slg_table builds one)")
    t = slg if isinstance(slg, th.Tensor) else th.tensor(list(slg), dtype=th.float32)
    t = t.detach().to("cpu", th.float32).reshape(-1).contiguous()
    if t.numel() != (n - 1) * stages:
        raise ValueError(f"{what} table has {t.numel()} entries, a {n}-point {method} grid has {(n - 1) * stages} stages")
    if not bool(th.isfinite(t).all()):
        raise ValueError(f"{what} table has an entry that is not finite")
    return t


def check_slg_layers(layers, n_layers=None):
    """the layer set as a list of ints; refused: an entry that is no integer, a repeated index, and - when the depth is known - an index
    outside ``0 .. n_layers - 1`` and a set that leaves no layer (what the engine refuses)"""
    out = []
    for v in (layers.reshape(-1).tolist() if isinstance(layers, th.Tensor) else list(layers)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"skip layer {v!r} is not an integer index")
        if int(v) in out:
            raise ValueError(f"skip index {int(v)} is repeated")
        out.append(int(v))
    if n_layers is not None:
        for v in out:
            if not 0 <= v < n_layers:
                raise ValueError(f"skip index {v} is outside 0..{n_layers - 1}")
        if len(out) >= n_layers:
            raise ValueError(f"the skip set leaves no layer (all {n_layers} are in it)")
    return out


def refuse_with_slg(slg, method="euler", rescale=0.0, norm_limit=math.inf, reuse=None):
    """what skip-layer guidance is not served with, by name: a rescale / norm-limit rule, a reuse table, a method that is not fixed-grid"""
    if slg is None:
        return
    if method not in FIXED_GRID_METHODS:
        raise ValueError(f"skip-layer guidance is built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not '{method}'")
    if not rule_is_off(rescale, norm_limit):
        raise ValueError("skip-layer guidance (an slg table) together with a rescale / norm_limit rule is not served")
    if reuse is not None:
        raise ValueError("skip-layer guidance (an slg table) together with guidance reuse (a reuse table) is not served")


def slg_combine(c, u, k, w, s):
    """the guided channels of one evaluation in bf16 tensor ops, every op rounding: ``(u + w (c - u)) + s (c - k)``, or - ``u`` None, the
    stage at ``w == 1`` - ``c + s (c - k)``.  ``c``, ``u``, ``k``: bf16 tensors; ``w``, ``s``: Python floats holding fp32 values"""
    if u is None:
        return c + s * (c - k)
    return (u + w * (c - u)) + s * (c - k)


def sample_cfg_slg(model, z, tgrid, table, slg, slg_layers, method="euler", *, cond=None, t_round=True, **kw):
    """The trajectory of skip-layer guidance on the host: every state ``[len(tgrid), *z.shape]``.  This IS the definition
    ``lt_sample_ode_cfg_slg`` is held to, state for state.  Per evaluation ``table`` gives the scale ``w`` and ``slg`` the skip-layer scale ``s``:

        s == 0            what sample_cfg_schedule does (forward_with_cfg at w, or the cond rows alone at w == 1)
        s != 0            k = bf16(model.forward(x[:B'], t[:B'], <cond half>, skip_layers=S))
                          o = bf16(model.forward(cat([x[:B']] * 2), t, <conditioning>))    (w == 1: the B' cond rows alone)
                          g = (u + w * (c - u)) + s * (c - k)                                (w == 1: g = c + s * (c - k))

    on the first ``min(model.cfg_channels, C)`` channels in bf16 tensor ops (every op rounds), the other channels passing through row by row
    (from the cond rows at ``w == 1``), ``g`` written to both halves, the result cast to the state dtype.  The loop is ``sample_cfg_schedule``'s,
    statement for statement."""
    if isinstance(z, (list, tuple)):
        raise ValueError("skip-layer guidance takes a tensor state; a packed batch (a list of latents) is not served")
    stages = _check_method(method)
    table = check_table(table, tgrid, method)
    slg = check_slg(slg, tgrid, method)
    layers = check_slg_layers(slg_layers, getattr(model, "n_layers", None))
    B = z.size(0)
    if B % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {B}")
    kw = dict(kw)
    kw.pop("cfg_scale", None)  # the table is the scale
    refuse_with_slg(slg, method, kw.pop("rescale", 0.0), kw.pop("norm_limit", math.inf), kw.pop("reuse", None))
    if cond is None:
        cond = [k for k, v in kw.items() if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] == B]
    cond_kw = {k: kw.pop(k) for k in cond}
    half_kw = {k: _cond_half(v, B) for k, v in cond_kw.items()}
    ch_model = int(getattr(model, "cfg_channels", 3))
    device = z.device
    t = _grid32(tgrid).to(device)
    w, sl = table.tolist(), slg.tolist()
    call = [0]

    def func(tt, y):
        scale, s = w[call[0]], sl[call[0]]
        call[0] += 1
        half = B // 2
        tvec = th.ones(B).to(device) * tt  # fp32 [B] (reference integrators.py:108)
        if s == 0.0:  # sample_cfg_schedule's stage
            if scale != 1.0:
                return model.forward_with_cfg(y, tvec, **cond_kw, cfg_scale=scale, **kw)
            o = model.forward(y[:half], tvec[:half], **half_kw)
            return th.cat([o, o])
        k = model.forward(y[:half], tvec[:half], **half_kw, skip_layers=layers).to(th.bfloat16)
        ch = min(ch_model, k.size(1))
        if scale != 1.0:
            o = model.forward(th.cat([y[:half]] * 2), tvec, **cond_kw).to(th.bfloat16)
            g = slg_combine(o[:half, :ch], o[half:, :ch], k[:, :ch], scale, s)
            return th.cat([th.cat([g, o[:half, ch:]], 1), th.cat([g, o[half:, ch:]], 1)]).to(y.dtype)
        o = model.forward(y[:half], tvec[:half], **half_kw).to(th.bfloat16)
        g = slg_combine(o[:, :ch], None, k[:, :ch], scale, s)
        r = th.cat([g, o[:, ch:]], 1)
        return th.cat([r, r]).to(y.dtype)

    def f(tt, y):
        return _call(func, tt, y) if t_round else func(tt, y)

    # fixed_grid_odeint's loop (integrators.py), statement for statement
    out = th.empty((len(t),) + tuple(z.shape), dtype=z.dtype, device=device)
    out[0] = z
    y = z
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    for j in range(len(t) - 1):
        t0, t1 = t[j], t[j + 1]
        dt = t1 - t0
        k1 = f(t0, y)
        if method == "euler":
            dy = dt * k1
        elif method == "midpoint":
            half = 0.5 * dt
            dy = dt * f(t0 + half, y + k1 * half)
        else:
            k2 = f(t0 + dt * third, y + dt * k1 * third)
            k3 = f(t0 + dt * two_thirds, y + dt * (k2 - k1 * third))
            k4 = f(t1, y + dt * (k1 - k2 + k3))
            dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        y = y + dy
        out[j + 1] = y
    assert call[0] == (len(t) - 1) * stages
    return out


# ---- perturbed-attention guidance: the third prediction runs a set of blocks with the identity as their attention map -----------
def pag_table(tgrid, method, pag_scale, interval=None):
    """The fp32 table of perturbed-attention scales of a trajectory, one per evaluation: ``slg_table``'s rule - ``pag_scale`` where
    ``lo <= t_stage < hi`` for ``interval = (lo, hi)`` (default: everywhere), 0 elsewhere, on the unrounded fp32 stage times"""
    return slg_table(tgrid, method, pag_scale, interval=interval, what="perturbed-attention")


def check_pag(pag, tgrid, method):
    """``pag`` as an fp32 CPU tensor of ``(len(tgrid) - 1) * stages`` finite entries"""
    if pag is None:
        raise ValueError("perturbed-attention table is None (one scale per evaluation; pag_table builds one)")
    return check_slg(pag, tgrid, method, what="perturbed-attention")


def check_pag_layers(pag_layers, skip_layers=(), n_layers=None, name="perturb"):
    """-> (perturb set, skip set) as lists of ints.  Refused: an entry that is no integer, a repeated index, an index in both sets, and -
    when the depth is known - an index outside ``0 .. n_layers - 1`` and a SKIP set that leaves no layer (the perturb set may hold every
    layer): what the engine refuses"""
    skip = check_slg_layers(skip_layers if skip_layers is not None else (), n_layers)
    out = []
    for v in (pag_layers.reshape(-1).tolist() if isinstance(pag_layers, th.Tensor) else list(pag_layers if pag_layers is not None else ())):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} layer {v!r} is not an integer index")
        if int(v) in out:
            raise ValueError(f"{name} index {int(v)} is repeated")
        if n_layers is not None and not 0 <= int(v) < n_layers:
            raise ValueError(f"{name} index {int(v)} is outside 0..{n_layers - 1}")
        if int(v) in skip:
            raise ValueError(f"layer {int(v)} is in the skip set and in the {name} set (the sets are disjoint)")
        out.append(int(v))
    return out, skip


def refuse_with_pag(pag, method="euler", rescale=0.0, norm_limit=math.inf, reuse=None, slg=None, teacache=None, mask=None,
                    what="perturbed-attention guidance", table="a pag table", layers="pag_layers"):
    """what perturbed-attention guidance is not served with, by name: the companions skip-layer guidance refuses - a rescale / norm-limit rule,
    a reuse table, a method that is not fixed-grid (multistep and adaptive solvers), step caching, an inpainting mask - and a second scale
    table (``slg`` beside ``pag``: the skip set joins the ONE third prediction under the ``pag`` table)"""
    if pag is None:
        return
    if slg is not None:
        raise ValueError(f"{what} ({table}) together with an slg table is not served: one third prediction, one scale "
                         f"table - give slg_layers beside {layers} under the {table[2:]}")
    if method not in FIXED_GRID_METHODS:
        raise ValueError(f"{what} is built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not '{method}'")
    if not rule_is_off(rescale, norm_limit):
        raise ValueError(f"{what} ({table}) together with a rescale / norm_limit rule is not served")
    if reuse is not None:
        raise ValueError(f"{what} ({table}) together with guidance reuse (a reuse table) is not served")
    if teacache is not None:
        raise ValueError(f"{what} ({table}) together with step caching (teacache) is not served")
    if mask is not None:
        raise ValueError(f"{what} ({table}) together with an inpainting mask is not served")


def sample_cfg_pag(model, z, tgrid, table, pag, pag_layers, skip_layers=(), method="euler", *, cond=None, t_round=True, **kw):
    """The trajectory of perturbed-attention guidance on the host: every state ``[len(tgrid), *z.shape]``.  This IS the definition
    ``lt_sample_ode_cfg_pag`` is held to, state for state.  Per evaluation ``table`` gives the scale ``w`` and ``pag`` the scale ``s``:

        s == 0            what sample_cfg_schedule does (forward_with_cfg at w, or the cond rows alone at w == 1)
        s != 0            k = bf16(model.forward(x[:B'], t[:B'], <cond half>, skip_layers=S, perturb_layers=P))
                          o = bf16(model.forward(cat([x[:B']] * 2), t, <conditioning>))    (w == 1: the B' cond rows alone)
                          g = (u + w * (c - u)) + s * (c - k)                                (w == 1: g = c + s * (c - k))

    ``P``: the blocks whose self-attention map is replaced by the identity (every query's output is its own value row; the text
    cross-attention stays), ``S``: the blocks left out; disjoint, either may be empty.  Everything else is ``sample_cfg_slg``, statement for
    statement: the chain of roundings is ``slg_combine``."""
    if isinstance(z, (list, tuple)):
        raise ValueError("perturbed-attention guidance takes a tensor state; a packed batch (a list of latents) is not served")
    stages = _check_method(method)
    table = check_table(table, tgrid, method)
    pag = check_pag(pag, tgrid, method)
    perturb, layers = check_pag_layers(pag_layers, skip_layers, getattr(model, "n_layers", None))
    if not perturb and not layers and bool((pag != 0).any()):
        raise ValueError("both layer sets are empty and the table has a non-zero scale: the third prediction would be the conditional one")
    B = z.size(0)
    if B % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {B}")
    kw = dict(kw)
    kw.pop("cfg_scale", None)  # the table is the scale
    refuse_with_pag(pag, method, kw.pop("rescale", 0.0), kw.pop("norm_limit", math.inf), kw.pop("reuse", None))
    return _sample_third(model, z, tgrid, table, pag, dict(skip_layers=layers, perturb_layers=perturb), method, stages, cond, t_round, kw)


def _sample_third(model, z, tgrid, table, s_table, third_kw, method, stages, cond, t_round, kw):
    """the loop ``sample_cfg_pag`` and ``sample_cfg_seg`` share: ``third_kw`` are the keywords that make ``model.forward`` the third
    prediction (the layer sets; the blur width), ``s_table`` its checked scale table, ``kw`` the caller's keywords with the refused ones taken
    out.  Everything is ``sample_cfg_slg``, statement for statement"""
    B = z.size(0)
    if cond is None:
        cond = [k for k, v in kw.items() if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] == B]
    cond_kw = {k: kw.pop(k) for k in cond}
    half_kw = {k: _cond_half(v, B) for k, v in cond_kw.items()}
    ch_model = int(getattr(model, "cfg_channels", 3))
    device = z.device
    t = _grid32(tgrid).to(device)
    w, sl = table.tolist(), s_table.tolist()
    call = [0]

    def func(tt, y):
        scale, s = w[call[0]], sl[call[0]]
        call[0] += 1
        half = B // 2
        tvec = th.ones(B).to(device) * tt  # fp32 [B] (reference integrators.py:108)
        if s == 0.0:  # sample_cfg_schedule's stage
            if scale != 1.0:
                return model.forward_with_cfg(y, tvec, **cond_kw, cfg_scale=scale, **kw)
            o = model.forward(y[:half], tvec[:half], **half_kw)
            return th.cat([o, o])
        k = model.forward(y[:half], tvec[:half], **half_kw, **third_kw).to(th.bfloat16)
        ch = min(ch_model, k.size(1))
        if scale != 1.0:
            o = model.forward(th.cat([y[:half]] * 2), tvec, **cond_kw).to(th.bfloat16)
            g = slg_combine(o[:half, :ch], o[half:, :ch], k[:, :ch], scale, s)
            return th.cat([th.cat([g, o[:half, ch:]], 1), th.cat([g, o[half:, ch:]], 1)]).to(y.dtype)
        o = model.forward(y[:half], tvec[:half], **half_kw).to(th.bfloat16)
        g = slg_combine(o[:, :ch], None, k[:, :ch], scale, s)
        r = th.cat([g, o[:, ch:]], 1)
        return th.cat([r, r]).to(y.dtype)

    def f(tt, y):
        return _call(func, tt, y) if t_round else func(tt, y)

    # fixed_grid_odeint's loop (integrators.py), statement for statement
    out = th.empty((len(t),) + tuple(z.shape), dtype=z.dtype, device=device)
    out[0] = z
    y = z
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    for j in range(len(t) - 1):
        t0, t1 = t[j], t[j + 1]
        dt = t1 - t0
        k1 = f(t0, y)
        if method == "euler":
            dy = dt * k1
        elif method == "midpoint":
            half = 0.5 * dt
            dy = dt * f(t0 + half, y + k1 * half)
        else:
            k2 = f(t0 + dt * third, y + dt * k1 * third)
            k3 = f(t0 + dt * two_thirds, y + dt * (k2 - k1 * third))
            k4 = f(t1, y + dt * (k1 - k2 + k3))
            dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        y = y + dy
        out[j + 1] = y
    assert call[0] == (len(t) - 1) * stages
    return out


# ---- smoothed-energy guidance: the third prediction runs a set of blocks on Gaussian-blurred queries ---------------------------
SEG_MAX_RADIUS = 31  # LT_SEG_MAX_RADIUS


def seg_taps(sigma):
    """What a blur width stands for: ``(mode, radius, taps)``.  ``sigma`` is taken as the fp32 value the engine receives.  ``+inf``: mode 1
    (every image query becomes the mean query), radius 0, no taps.  Otherwise mode 0, ``radius = min(ceil(3 sigma), 31)`` and the
    ``2 radius + 1`` taps as an fp32 tensor: the Gaussian ``exp(-k^2 / (2 sigma^2))`` in float64 (``math.exp``), summed from ``k = -radius``
    upward, every tap divided by the sum and rounded once to fp32.  ``lt_op_seg_taps`` is held to this word for word."""
    sg = float(th.tensor(float(sigma), dtype=th.float32))
    if not sg > 0.0:
        raise ValueError(f"blur sigma {sigma!r} is not positive (+inf is the mean query)")
    if math.isinf(sg):
        return 1, 0, th.zeros(0, dtype=th.float32)
    r = int(min(math.ceil(3.0 * sg), SEG_MAX_RADIUS))
    den = 2.0 * sg * sg
    g = [math.exp(-float(k * k) / den) for k in range(-r, r + 1)]
    total = 0.0
    for v in g:
        total += v
    return 0, r, th.tensor([v / total for v in g], dtype=th.float64).to(th.float32)


def seg_table(tgrid, method, seg_scale, interval=None):
    """The fp32 table of smoothed-energy scales of a trajectory, one per evaluation: ``slg_table``'s rule"""
    return slg_table(tgrid, method, seg_scale, interval=interval, what="smoothed-energy")


def check_seg(seg, tgrid, method):
    """``seg`` as an fp32 CPU tensor of ``(len(tgrid) - 1) * stages`` finite entries"""
    if seg is None:
        raise ValueError("smoothed-energy table is None (one scale per evaluation; seg_table builds one)")
    return check_slg(seg, tgrid, method, what="smoothed-energy")


def check_seg_layers(seg_layers, skip_layers=(), n_layers=None):
    """-> (blur set, skip set) as lists of ints: ``check_pag_layers``' refusals with "blur" for "perturb" (the blur set may hold every layer)"""
    return check_pag_layers(seg_layers, skip_layers, n_layers, name="blur")


def refuse_with_seg(seg, method="euler", rescale=0.0, norm_limit=math.inf, reuse=None, slg=None, teacache=None, mask=None, pag=None):
    """what smoothed-energy guidance is not served with, by name: everything perturbed-attention guidance refuses, and ``pag`` itself (one
    third prediction, and no evaluation runs a blur set beside a perturb set)"""
    if seg is None:
        return
    if pag is not None:
        raise ValueError("smoothed-energy guidance (a seg table) together with perturbed-attention guidance (a pag table) is not served: one "
                         "third prediction, and no evaluation blurs and perturbs")
    refuse_with_pag(seg, method, rescale, norm_limit, reuse, slg, teacache, mask, what="smoothed-energy guidance", table="a seg table",
                    layers="seg_layers")


def sample_cfg_seg(model, z, tgrid, table, seg, seg_layers, seg_sigma, skip_layers=(), method="euler", *, cond=None, t_round=True, **kw):
    """The trajectory of smoothed-energy guidance on the host: every state ``[len(tgrid), *z.shape]``.  This IS the definition
    ``lt_sample_ode_cfg_seg`` is held to, state for state.  It is ``sample_cfg_pag`` with

        k = bf16(model.forward(x[:B'], t[:B'], <cond half>, skip_layers=S, blur_layers=Q, blur_sigma=sigma))

    as the third evaluation: the blocks of ``Q`` run their self-attention on queries blurred over the 2-D token grid (``seg_taps``; the
    post-RoPE queries; the text cross-attention reads the queries as they are), ``S``: the blocks left out; disjoint, either may be empty."""
    if isinstance(z, (list, tuple)):
        raise ValueError("smoothed-energy guidance takes a tensor state; a packed batch (a list of latents) is not served")
    stages = _check_method(method)
    table = check_table(table, tgrid, method)
    seg = check_seg(seg, tgrid, method)
    blur, layers = check_seg_layers(seg_layers, skip_layers, getattr(model, "n_layers", None))
    if blur:
        seg_taps(seg_sigma)
    if not blur and not layers and bool((seg != 0).any()):
        raise ValueError("both layer sets are empty and the table has a non-zero scale: the third prediction would be the conditional one")
    if z.size(0) % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {z.size(0)}")
    kw = dict(kw)
    kw.pop("cfg_scale", None)  # the table is the scale
    refuse_with_seg(seg, method, kw.pop("rescale", 0.0), kw.pop("norm_limit", math.inf), kw.pop("reuse", None))
    third_kw = dict(skip_layers=layers, blur_layers=blur, blur_sigma=seg_sigma)
    return _sample_third(model, z, tgrid, table, seg, third_kw, method, stages, cond, t_round, kw)


def sample_seg_front(x, model, tgrid, method, table, model_kwargs, seg, seg_layers, seg_sigma, slg_layers=(), *, t_round=True, use_engine=True,
                     project=None, compose=None, windows=None, **companions):
    """what ``ODE.sample`` / ``ode.sample`` do with ``seg_table=``: the refusals by name (``companions``: the keyword arguments of
    ``refuse_with_seg``; projected / composed guidance and windows besides), then ONE engine call for the bound ``forward_with_cfg`` of an
    engine-backed model on a ROCm state, else the host loop ``sample_cfg_seg``.  Without a table ``cfg_scale`` holds at every stage."""
    from .integrators import _engine_target
    if isinstance(x, (list, tuple)):
        raise ValueError("smoothed-energy guidance (seg_table) takes a tensor state; a packed batch (a list of latents) is not served")
    for given, name in ((project, "projected guidance (cfg_apg / cfg_zero_star)"), (compose, "composed guidance (compose)"),
                        (windows, "tiled sampling (windows)")):
        if given is not None:
            raise ValueError(f"smoothed-energy guidance (a seg table) together with {name} is not served")
    refuse_with_seg(seg, method, **companions)
    if seg_sigma is None:
        raise ValueError("smoothed-energy guidance: seg_table needs seg_sigma (> 0; inf: the mean query)")
    if table is None:
        table = cfg_table(tgrid, method, model_kwargs.get("cfg_scale", 1.0))
    target = _engine_target(model)
    if target is not None and target[1] and x.is_cuda and use_engine and hasattr(target[0], "_engine_sample_ode_cfg_schedule"):
        return target[0]._engine_sample_ode_cfg_schedule(x, tgrid, method, t_round, table, dict(model_kwargs), seg=seg, seg_layers=seg_layers,
                                                         seg_sigma=seg_sigma, slg_layers=slg_layers)
    owner = getattr(model, "__self__", None)
    if owner is None or getattr(model, "__name__", "") != "forward_with_cfg" or not hasattr(owner, "forward"):
        raise TypeError("seg_table needs the bound forward_with_cfg of a model that also has forward (the third evaluation calls it)")
    return sample_cfg_seg(owner, x, tgrid, table, seg, seg_layers, seg_sigma, slg_layers, method, t_round=t_round, **model_kwargs)


# ---- projected guidance: APG and CFG-Zero*, the forms that need inner products of the two predictions ---------------------------
PROJECT_FORMS = {"apg": 1, "zero_star": 2}  # LT_PROJECT_APG / LT_PROJECT_ZERO_STAR


def _f32(v):
    return float(th.tensor(float(v), dtype=th.float32))


def check_project(apg=None, zero_star=False, zero_init=0, n_grid=None):
    """``(form, eta, momentum, norm_threshold, zero_init)``: ``form`` None (off: neither given), ``"apg"`` or ``"zero_star"``; the three
    parameters as the fp32 values the engine reads, as Python floats.  ``apg``: a dict with any of ``eta`` (default 1), ``momentum``
    (default 0), ``norm_threshold`` (default inf: off).  Refused: both forms at once; an unknown key; ``eta`` not finite; ``|momentum| >= 1``;
    ``norm_threshold`` not above 0; ``zero_init`` without ``zero_star``, negative, no integer, or - when the grid is known - ``>= n_grid - 1``."""
    if isinstance(zero_init, bool) or int(zero_init) != zero_init:
        raise ValueError(f"zero_init {zero_init!r} is not an integer count of grid intervals")
    zero_init = int(zero_init)
    if zero_init < 0:
        raise ValueError(f"zero_init {zero_init} is negative")
    if apg is not None and zero_star:
        raise ValueError("APG (apg=...) and CFG-Zero* (zero_star) are exclusive: one projected form per call")
    if zero_init and not zero_star:
        raise ValueError(f"zero_init {zero_init} belongs to CFG-Zero* (zero_star=True)")
    if n_grid is not None and zero_init >= n_grid - 1 and zero_init:
        raise ValueError(f"zero_init {zero_init} leaves no interval of the {n_grid - 1} to integrate")
    if apg is None:
        return ("zero_star" if zero_star else None), 1.0, 0.0, math.inf, zero_init
    apg = dict(apg)
    unknown = sorted(set(apg) - {"eta", "momentum", "norm_threshold"})
    if unknown:
        raise ValueError(f"apg takes eta, momentum and norm_threshold, not {unknown}")
    eta, beta, r = float(apg.get("eta", 1.0)), float(apg.get("momentum", 0.0)), float(apg.get("norm_threshold", math.inf))
    if not math.isfinite(eta):
        raise ValueError(f"apg eta {eta} is not finite")
    if not abs(beta) < 1.0:
        raise ValueError(f"apg momentum {beta} is not inside (-1, 1)")
    if math.isnan(r) or not r > 0.0:
        raise ValueError(f"apg norm_threshold {r} is not above 0 (inf switches the clip off)")
    eta, beta, r = _f32(eta), _f32(beta), _f32(r)
    if not abs(beta) < 1.0:  # (a value that rounds to 1 in fp32)
        raise ValueError(f"apg momentum {beta} is not inside (-1, 1) as an fp32 value")
    return "apg", eta, beta, r, zero_init


def refuse_with_project(form, method="euler", rescale=0.0, norm_limit=math.inf, reuse=None, slg=None, pag=None, teacache=None, mask=None,
                        packed=False):
    """what a projected form is not served with, by name: a rescale / norm-limit rule, a reuse table, skip-layer and perturbed-attention
    guidance, step caching, an inpainting mask, a packed batch, and a method that is not fixed-grid - the multistep solvers (zero velocity and
    the slope ring are not defined together) and the adaptive ones"""
    if form is None:
        return
    what = "projected guidance (APG)" if form == "apg" else "projected guidance (CFG-Zero*)"
    if packed:
        raise ValueError(f"{what}: a packed batch (a list of latents) is not served")
    if method not in FIXED_GRID_METHODS:
        raise ValueError(f"{what} is built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not '{method}'")
    if not rule_is_off(rescale, norm_limit):
        raise ValueError(f"{what} together with a rescale / norm_limit rule is not served")
    for name, v in (("guidance reuse (a reuse table)", reuse), ("skip-layer guidance (an slg table)", slg),
                    ("perturbed-attention guidance (a pag table)", pag), ("step caching (teacache)", teacache), ("an inpainting mask", mask)):
        if v is not None:
            raise ValueError(f"{what} together with {name} is not served")


def apg_coefficients(Smm, Smc, Scc, w, eta, norm_threshold):
    """``(a, b, tn, p)`` of one sample from its three float64 sums: float64 arithmetic operation by operation (Python floats: no fused
    multiply-add), ``a`` and ``b`` each rounded once to fp32"""
    tn = min(1.0, norm_threshold / math.sqrt(Smm)) if (norm_threshold < math.inf and Smm > 0.0) else 1.0
    p = tn * Smc / Scc if Scc > 0.0 else 0.0
    w1 = w - 1.0
    return _f32(w1 * tn), _f32(w1 * (eta - 1.0) * p), tn, p


def guided_project(o, w, ch, form, *, eta=1.0, momentum=0.0, norm_threshold=math.inf, m_prev=None, sums=None, parts=None):
    """A projected form at scale ``w`` on a model output ``o [B, C, H, W]`` (cond rows ``c``, then uncond rows ``u``; taken as bf16, returned in
    its own dtype): ``(out, coef, m)``.  Sums run over a sample's ``ch H W`` guided elements in float64; the coefficients are float64 scalar
    arithmetic, each rounded once to fp32; every tensor operation rounds on its own.  ``w`` and the parameters are taken as fp32 values.

    ``form="apg"`` (Sadat et al. 2024): ``d = bf16(c - u)``; ``m = d + momentum * m_prev`` in fp32 (``m_prev [B / 2, ch, H, W]``, None: zeros)
    is the returned state; ``tn = min(1, r / |m|)``, ``p = tn <m, c> / <c, c>``, ``a = fp32((w - 1) tn)``, ``b = fp32((w - 1)(eta - 1) p)``
    (``apg_coefficients``); ``g = bf16(c + (a m + b c))``.  This is ``c + (w - 1)(orth + eta par)`` of the published algorithm with
    ``par = (<m', c> / <c, c>) c`` and ``m' = tn m`` - the projection is taken on the model's VELOCITY output, where the paper takes it on the
    denoised prediction; for this family's linear path the two differ by a multiple of the state, and the velocity is what the engine holds.
    With ``eta = 1, momentum = 0, r = inf`` it is ``c + (w - 1)(c - u)``: plain guidance in another rounding chain - NOT the words of
    ``forward_with_cfg`` / lt_forward_cfg, which form ``u + w (c - u)`` in bf16 steps.
    ``form="zero_star"`` (Fan et al. 2025): ``s = fp32(<c, u> / <u, u>)`` (1 where ``<u, u>`` is 0); ``g = bf16(s u + w (c - s u))``; ``m`` is None.

    ``g`` goes to both halves; the channels past ``ch`` pass through row by row.  ``coef``: fp32 ``[B / 2, 2]`` (a, b), or ``[B / 2]`` s, on
    ``o``'s device.  ``sums`` (a list of per-sample tuples - (Smm, Smc, Scc) or (Scu, Suu)): taken in place of the reductions here;
    ``parts`` (a list): receives per sample ``(Smm, Smc, Scc, tn, p)`` or ``(Scu, Suu)``."""
    if form not in PROJECT_FORMS:
        raise ValueError(f"projected form {form!r} is not one of {sorted(PROJECT_FORMS)}")
    B = o.size(0)
    if B % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {B}")
    half = B // 2
    ch = min(int(ch), o.size(1))
    dtype = o.dtype
    w = _f32(w)
    o = o.to(th.bfloat16)  # the model's output is bf16 (an engine-backed model hands an fp32 state the same values in fp32)
    c, u = o[:half, :ch], o[half:, :ch]
    cf = c.float()
    if form == "apg":
        _, eta, beta, r, _ = check_project(dict(eta=eta, momentum=momentum, norm_threshold=norm_threshold))
        d = c - u
        m_prev = th.zeros(d.shape, dtype=th.float32, device=o.device) if m_prev is None else m_prev.to(o.device, th.float32)
        m = d.float() + beta * m_prev  # (from zeros too: the same two operations, so the same signed zeros)
        if sums is None:
            md, cd = m.double().reshape(half, -1), c.double().reshape(half, -1)
            sums = th.stack([(md * md).sum(1), (md * cd).sum(1), (cd * cd).sum(1)], dim=1).tolist()
        coef = []
        for Smm, Smc, Scc in sums:
            a, b, tn, p = apg_coefficients(Smm, Smc, Scc, w, eta, r)
            coef.append((a, b))
            if parts is not None:
                parts.append((Smm, Smc, Scc, tn, p))
        coef = th.tensor(coef, dtype=th.float32, device=o.device).reshape(half, 2)
        a, b = coef[:, 0].view(-1, 1, 1, 1), coef[:, 1].view(-1, 1, 1, 1)
        gg = (cf + (a * m + b * cf)).to(th.bfloat16)
    else:
        m = None
        if sums is None:
            cd, ud = c.double().reshape(half, -1), u.double().reshape(half, -1)
            sums = th.stack([(cd * ud).sum(1), (ud * ud).sum(1)], dim=1).tolist()
        coef = []
        for Scu, Suu in sums:
            coef.append(_f32(Scu / Suu if Suu > 0.0 else 1.0))
            if parts is not None:
                parts.append((Scu, Suu))
        coef = th.tensor(coef, dtype=th.float32, device=o.device)
        su = coef.view(-1, 1, 1, 1) * u.float()
        gg = (su + w * (cf - su)).to(th.bfloat16)
    out = th.cat([th.cat([gg, o[:half, ch:]], 1), th.cat([gg, o[half:, ch:]], 1)])
    return out.to(dtype), coef, m


def sample_cfg_project(model, z, tgrid, table, method="euler", *, apg=None, zero_star=False, zero_init=0, cond=None, t_round=True,
                       factors=None, parts=None, calls=None, **kw):
    """``sample_cfg_schedule`` whose stages at a scale other than 1 run ``guided_project`` on ``model.forward`` of all ``B`` rows (both halves
    of the input are the first half, as ``forward_with_cfg`` makes them); a stage at scale 1 exactly is the conditional-only stage and leaves
    the momentum alone.  This IS the definition ``lt_sample_ode_cfg_project`` is held to, state for state.  APG's momentum is zero at the start
    of the call and advances with every guided evaluation, in evaluation order (the stages of midpoint / rk4 count).  ``zero_init = K``
    (CFG-Zero*): the first ``K`` grid intervals take zero velocity - the state is copied into their slots, the model is not called and their
    table entries are not read.  ``factors`` (a list): receives the coefficient tensor of every guided stage, ``parts`` (a list) what
    ``guided_project`` reports per sample; ``calls`` (a list): receives the number of model calls."""
    stages = _check_method(method)
    table = check_table(table, tgrid, method)
    form, eta, beta, r, zero_init = check_project(apg, zero_star, zero_init, n_grid=len(_grid32(tgrid)))
    if form is None:
        raise ValueError("sample_cfg_project needs a projected form: apg=dict(...) or zero_star=True")
    B = z.size(0)
    if B % 2:
        raise ValueError(f"guidance needs an even batch (cond + uncond rows), got {B}")
    kw = dict(kw)
    kw.pop("cfg_scale", None)  # the table is the scale
    refuse_with_project(form, method, kw.pop("rescale", 0.0), kw.pop("norm_limit", math.inf), kw.pop("reuse", None))
    if cond is None:
        cond = [k for k, v in kw.items() if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] == B]
    cond_kw = {k: kw.pop(k) for k in cond}
    half_kw = {k: _cond_half(v, B) for k, v in cond_kw.items()}
    ch = int(getattr(model, "cfg_channels", 3))
    device = z.device
    t = _grid32(tgrid).to(device)
    w = table.tolist()
    call = [zero_init * stages]
    made = [0]
    mom = [None]

    def func(tt, y):
        scale = w[call[0]]
        call[0] += 1
        made[0] += 1
        tvec = th.ones(B).to(device) * tt  # fp32 [B] (reference integrators.py:108)
        if scale != 1.0:
            o = model.forward(th.cat([y[: B // 2]] * 2), tvec, **cond_kw)
            out, coef, m = guided_project(o, scale, ch, form, eta=eta, momentum=beta, norm_threshold=r, m_prev=mom[0], parts=parts)
            mom[0] = m
            if factors is not None:
                factors.append(coef)
            return out.to(y.dtype)
        o = model.forward(y[: B // 2], tvec[: B // 2], **half_kw)
        return th.cat([o, o])

    def f(tt, y):
        return _call(func, tt, y) if t_round else func(tt, y)

    # fixed_grid_odeint's loop (integrators.py), statement for statement - behind the intervals of zero velocity
    out = th.empty((len(t),) + tuple(z.shape), dtype=z.dtype, device=device)
    out[0] = z
    y = z
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    for j in range(len(t) - 1):
        if j < zero_init:  # y + dt * 0
            out[j + 1] = y
            continue
        t0, t1 = t[j], t[j + 1]
        dt = t1 - t0
        k1 = f(t0, y)
        if method == "euler":
            dy = dt * k1
        elif method == "midpoint":
            half = 0.5 * dt
            dy = dt * f(t0 + half, y + k1 * half)
        else:
            k2 = f(t0 + dt * third, y + dt * k1 * third)
            k3 = f(t0 + dt * two_thirds, y + dt * (k2 - k1 * third))
            k4 = f(t1, y + dt * (k1 - k2 + k3))
            dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        y = y + dy
        out[j + 1] = y
    assert call[0] == (len(t) - 1) * stages and made[0] == (len(t) - 1 - zero_init) * stages
    if calls is not None:
        calls.append(made[0])
    return out


def sample_project_front(x, model, tgrid, method, table, model_kwargs, *, apg=None, zero_star=False, zero_init=0, t_round=True, use_engine=True,
                         **companions):
    """what ``ODE.sample`` / ``ode.sample`` do with ``cfg_apg=`` / ``cfg_zero_star=`` / ``cfg_zero_init=``: the refusals by name
    (``companions``: the keyword arguments of ``refuse_with_project``), then ONE engine call for the bound ``forward_with_cfg`` of an
    engine-backed model on a ROCm state, else the host loop ``sample_cfg_project``.  Without a table ``cfg_scale`` holds at every stage."""
    from .integrators import _engine_target
    if isinstance(x, tuple):
        raise NotImplementedError("tuple states are not part of the sampling path of projected guidance")
    form = check_project(apg, zero_star, zero_init, n_grid=len(_grid32(tgrid)))[0]
    refuse_with_project(form, method, packed=isinstance(x, list), **companions)
    if table is None:
        table = cfg_table(tgrid, method, model_kwargs.get("cfg_scale", 1.0))
    target = _engine_target(model)
    if target is not None and target[1] and x.is_cuda and use_engine and hasattr(target[0], "_engine_sample_ode_cfg_schedule"):
        return target[0]._engine_sample_ode_cfg_schedule(x, tgrid, method, t_round, table, dict(model_kwargs), apg=apg, zero_star=zero_star,
                                                         zero_init=zero_init)
    owner = getattr(model, "__self__", None)
    if owner is None or getattr(model, "__name__", "") != "forward_with_cfg" or not hasattr(owner, "forward"):
        raise TypeError("projected guidance needs the bound forward_with_cfg of a model that also has forward (every stage calls it)")
    return sample_cfg_project(owner, x, tgrid, table, method, apg=apg, zero_star=zero_star, zero_init=zero_init, t_round=t_round, **model_kwargs)


# ---- composed guidance -----------------------------------------------------------------------------------------------------
COMPOSE_MAX = 7  # prompts beside the base prompt (LT_COMPOSE_MAX); the engine's row budget is (K + 1) B' <= max_batch <= 8


def check_compose(weights, K=None, rows=None):
    """``weights`` as an fp32 CPU tensor ``[rows, K]`` of finite entries (a 1-D table is one row); ``K`` / ``rows``: what it must have"""
    w = weights if isinstance(weights, th.Tensor) else th.tensor(weights, dtype=th.float32)
    w = w.detach().to("cpu", th.float32)
    if w.dim() == 1:
        w = w[None]
    if w.dim() != 2 or w.shape[0] < 1:
        raise ValueError(f"composed guidance: the weights must be [K] or [stages, K], got {tuple(w.shape)}")
    if not 1 <= w.shape[1] <= COMPOSE_MAX:
        raise ValueError(f"composed guidance: K = {w.shape[1]} prompts (1 .. {COMPOSE_MAX})")
    if K is not None and w.shape[1] != K:
        raise ValueError(f"composed guidance: the weights are for {w.shape[1]} prompts, the call has K = {K}")
    if rows is not None and w.shape[0] != rows:
        raise ValueError(f"composed guidance: the weight table has {w.shape[0]} rows, the grid has {rows} stages")
    if not bool(th.isfinite(w).all()):
        raise ValueError("composed guidance: a weight is not finite")
    return w.contiguous()


def compose_table(tgrid, method, weights, intervals=None):
    """The fp32 weight table ``[(len(tgrid) - 1) * stages, K]`` of a composed trajectory: stage ``k`` of interval ``i`` uses row
    ``i * stages + k``.  ``weights``: the K weights.  ``intervals[k] = (lo, hi)`` (``None``: everywhere) sets prompt ``k``'s weight to 0 where
    not ``lo <= t_stage < hi`` - ``cfg_table``'s test, on the UNROUNDED fp32 stage time."""
    _check_method(method)
    w = check_compose(weights)
    if w.shape[0] != 1:
        raise ValueError("compose_table takes the K weights of the prompts, one each")
    K = w.shape[1]
    ts = stage_times(tgrid, method, th.float32, False).tolist()
    intervals = [None] * K if intervals is None else list(intervals)
    if len(intervals) != K:
        raise ValueError(f"compose_table: {len(intervals)} intervals for K = {K} prompts (one each; None: everywhere)")
    table = w.repeat(len(ts), 1)
    for k, iv in enumerate(intervals):
        if iv is None:
            continue
        lo, hi = float(iv[0]), float(iv[1])
        if not lo <= hi:
            raise ValueError(f"guidance interval [{lo}, {hi}) of prompt {k} is empty or not ordered")
        for i, t in enumerate(ts):
            if not lo <= t < hi:
                table[i, k] = 0.0
    return table.contiguous()


def guided_compose(outs, weights, cfg_channels=3):
    """The composed output ``[B', C, H, W]`` of one plain ``forward`` of ``(K + 1) B'`` rows ``outs``: rows ``k B' + b`` belong to prompt ``k`` of
    image ``b`` (``k = 0 .. K-1``), rows ``K B' + b`` to the base prompt.  On channels ``< cfg_channels``, with R = round to bf16 - the model's
    output dtype, whatever the dtype ``outs`` arrives in - and every difference, product and sum one fp32 operation that rounds on its own::

        acc = R(w_1 * R(c_1 - u))
        acc = R(acc + R(w_k * R(c_k - u)))    for k = 2 .. K, in this order
        g   = R(u + acc)

    (torch's bf16 elementwise kernels compute in fp32 and round once; a Python float weight enters as its fp32 value).  At ``K = 1`` this is
    ``forward_with_cfg``'s ``u + w * (c - u)``.  Channels at or past ``cfg_channels`` are prompt 1's rows, copied."""
    w = check_compose(weights)
    if w.shape[0] != 1:
        raise ValueError("guided_compose takes the K weights of ONE evaluation")
    K = w.shape[1]
    if outs.dim() != 4 or outs.shape[0] % (K + 1):
        raise ValueError(f"guided_compose: {outs.shape[0]} rows are not a multiple of K + 1 = {K + 1} (K prompt rows and the base row per image)")
    C = outs.shape[1]
    if not 1 <= int(cfg_channels) <= C:
        raise ValueError(f"composed guidance: cfg_channels {cfg_channels} outside 1..{C}")
    ch = int(cfg_channels)
    rows = outs.to(th.bfloat16).chunk(K + 1)
    u = rows[K][:, :ch]
    wk = w[0].tolist()
    acc = wk[0] * (rows[0][:, :ch] - u)
    for k in range(1, K):
        acc = acc + wk[k] * (rows[k][:, :ch] - u)
    g = u + acc
    return th.cat([g, rows[0][:, ch:]], 1).to(outs.dtype)


def sample_cfg_compose(model_fn, z, tgrid, table, K, method="euler", *, cfg_channels=3, **cond_kw):
    """The composed trajectory on the host: all ``len(tgrid)`` states ``[len(tgrid), B', C, H, W]``.  The stepping is ``fixed_grid_odeint`` itself
    - the stage times, the dt handling and every rounding point of the loop ``lt_sample_ode`` is pinned to - and its velocity is: the ``B'`` state
    rows replicated ``K + 1`` times, ONE ``model_fn(rows, t fp32 [(K + 1) B'], **cond_kw)`` (a plain forward whose conditioning carries the rows
    of ``guided_compose``'s layout), ``guided_compose`` with row ``i * stages + k`` of ``table`` at stage ``k`` of interval ``i``."""
    stages = _check_method(method)
    K = int(K)
    t = _grid32(tgrid)
    table = check_compose(table, K, (len(t) - 1) * stages)
    if z.dim() != 4:
        raise ValueError(f"composed guidance takes a state [B', C, H, W], got {tuple(z.shape)}")
    rows = (K + 1) * z.shape[0]
    for k, v in cond_kw.items():
        if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] != rows:
            raise ValueError(f"composed guidance: conditioning '{k}' has {v.shape[0]} rows; {z.shape[0]} image(s) under K = {K} prompts need "
                             f"(K + 1) B' = {rows} rows (prompt 1's, ..., prompt K's, the base prompt's)")
    device = z.device
    w = table.tolist()
    call = [0]

    def _fn(tt, y):
        wk = w[call[0]]
        call[0] += 1
        tvec = th.ones(rows).to(device) * tt  # fp32 [(K + 1) B'] (reference integrators.py:108)
        return guided_compose(model_fn(y.repeat(K + 1, 1, 1, 1), tvec, **cond_kw), wk, cfg_channels)

    out = fixed_grid_odeint(_fn, z, t.to(device), method=method)
    assert call[0] == (len(t) - 1) * stages
    return out


# what the composed call does not combine with, refused by name in the Python wrappers (the C entries take none of them)
def refuse_with_compose(method, **others):
    """``others``: name -> value of the features a call was given beside ``compose``; any that is set is refused by name"""
    names = {"cfg_table": "a guidance table (cfg_table)", "rule": "a rescale / norm limit (cfg_rescale, cfg_norm_limit)",
             "cfg_reuse": "guidance reuse (cfg_reuse)", "slg": "skip-layer guidance (slg_table)", "pag": "perturbed-attention guidance (pag_table)",
             "project": "projected guidance (cfg_apg, cfg_zero_star)", "teacache": "step caching (teacache)", "mask": "an inpainting mask",
             "windows": "tiled sampling (windows)", "packed": "a packed batch (a list of latents)"}
    for key, v in others.items():
        if v is not None and v is not False:
            raise NotImplementedError(f"composed guidance (compose) and {names.get(key, key)} are not served together")
    if method not in FIXED_GRID_METHODS:
        raise NotImplementedError(f"composed guidance (compose) is built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not '{method}' "
                                  "(the multistep and adaptive solvers are not served)")


def sample_compose_front(x, model, tgrid, method, model_kwargs, table, *, t_round=True, use_engine=True, **others):
    """``sample(..., compose=table)`` of both ODE front ends: the refusals by name, then ONE ``lt_sample_ode_compose`` call for an engine-backed
    model on a ROCm state, the host loop ``sample_cfg_compose`` around the plain ``forward`` otherwise.  ``x [B', C, H, W]``; ``table``
    ``[stages, K]`` (``compose_table``); the conditioning in ``model_kwargs`` carries ``(K + 1) B'`` rows.  ``model``: the bound ``forward`` or
    ``forward_with_cfg`` of the model (the step flags of the latter reach the engine; ``cfg_scale`` is ignored: the table holds the weights)."""
    from .integrators import _engine_target
    refuse_with_compose(method, packed=True if isinstance(x, (list, tuple)) else None, **others)
    table = check_compose(table)
    K = table.shape[1]
    kw = dict(model_kwargs)
    kw.pop("cfg_scale", None)
    target = _engine_target(model)
    if target is not None and x.is_cuda and use_engine and hasattr(target[0], "_engine_sample_ode_compose"):
        return target[0]._engine_sample_ode_compose(x, tgrid, method, t_round, table, kw)
    owner = getattr(model, "__self__", None)
    fn = owner.forward if owner is not None and getattr(model, "__name__", "") == "forward_with_cfg" and hasattr(owner, "forward") else model
    rows = (K + 1) * x.shape[0]
    cond = {k: v for k, v in kw.items() if isinstance(v, th.Tensor) and v.dim() >= 1 and v.shape[0] == rows}
    if len(cond) != len(kw):
        raise TypeError(f"composed guidance: the host loop's plain forward takes the conditioning of {rows} rows alone, not {sorted(set(kw) - set(cond))}")
    return sample_cfg_compose(fn, x, tgrid, table, K, method, **cond)
