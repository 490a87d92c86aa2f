"""ODE / SDE integrators of the transport sampler (API mirror of ``lumina_next_t2i/transport/integrators.py``).

The reference delegates ODE stepping to ``torchdiffeq.odeint`` (integrators.py:115; third party, unpinned,
not vendored).  Here:

* when the model callable is a bound ``forward_with_cfg`` / ``forward`` of our engine-backed ``NextDiT`` and
  the drift is the plain velocity field, the whole trajectory runs inside the C-ABI engine
  (``lt_sample_ode``: one host loop in C++, no Python per step, no device syncs);
* for any other callable the fixed-grid solvers of torchdiffeq (euler / midpoint / rk4 "3/8 rule") are
  restated below in plain torch ops on whatever device the state lives on.  This is host glue for the
  model-callable protocol (transport.py:192-195), not a fallback of the HIP path;
* ``dopri5`` (the default ``--solver`` of ``Next-DiT-ImageNet/sample.py:48`` and of ``Sampler.sample_ode``,
  transport.py:349) is torchdiffeq's adaptive Dormand-Prince 5(4) solver, restated below: the step-size controller
  lives on the host (one scalar device->host read per attempted step is inherent to adaptive stepping).  With an
  engine-backed bound method, the plain velocity as drift and a bf16 / fp32 state on the GPU the whole loop is ONE
  C-ABI call (``lt_sample_ode_adaptive``: fused stage / error / norm / dense-output kernels, the controller in C++);
  ``solver.use_engine = False`` keeps the host loop below, which every other callable, tuple states and CPU states run anyway.
  The engine's error norm is a float64 tree sum rounded once to fp32, the host loop's is torch's fp32 reduction: dt may differ by
  fp32 ulps between the two and the step sequences may drift apart.  PARITY UNPINNED like the fixed-grid
  solvers (torchdiffeq is neither vendored nor installed); anchored on closed-form ODEs in the tests;
* the other tableau-defined methods ``--solver`` can name (the reference forwards ANY torchdiffeq method string,
  ``lumina_next_t2i/sample.py:77`` -> ``integrators.py:115``): fixed-grid ``heun2`` / ``heun3`` and adaptive ``bosh3`` /
  ``fehlberg2`` / ``adaptive_heun`` run on the same two host loops with their Butcher tableaus (restated from torchdiffeq 0.2.x,
  unpinned like the rest).  ``dopri8``, torchdiffeq's Adams family (``explicit_adams`` / ``implicit_adams`` / ``fixed_adams``) and ``scipy_solver`` are NOT built and say
  so by name;
* the linear multistep methods ``ab2`` / ``ab3`` / ``abm2`` / ``abm3`` (``transport/multistep.py``: variable-step Adams-Bashforth predictors, with
  an Adams-Moulton corrector that costs no evaluation; ONE model evaluation per grid interval) are this project's own, not torchdiffeq's: one
  ``lt_sample_ode_multistep`` call for an engine-backed callable, ``multistep_odeint`` otherwise or with ``use_engine = False``.

The SDE samplers (``class sde``: Euler-Maruyama / Heun, the reference's own code) run inside the engine as well when the model callable is
engine-backed and predicts a velocity (``lt_sample_sde``: one evaluation per stage, coefficients from ``sde_table``); otherwise through the
model callable, step by step, as the reference does.
"""
import math

import torch as th

from .multistep import MULTISTEP_METHODS, multistep_odeint  # ab2 / ab3 / abm2 / abm3: ours, not torchdiffeq's Adams family

FIXED_GRID_METHODS = ("euler", "midpoint", "rk4")           # also built inside the engine (lt_sample_ode): one C-ABI call per trajectory
HOST_FIXED_GRID_METHODS = ("heun2", "heun3")                  # fixed grid, host loop only
ADAPTIVE_METHODS = ("dopri5", "bosh3", "fehlberg2", "adaptive_heun")  # also inside the engine (lt_sample_ode_adaptive)
NOT_BUILT_METHODS = ("dopri8", "explicit_adams", "implicit_adams", "fixed_adams", "scipy_solver")
ALL_METHODS = FIXED_GRID_METHODS + HOST_FIXED_GRID_METHODS + ADAPTIVE_METHODS  # the torchdiffeq names built here
BUILT_METHODS = ALL_METHODS + MULTISTEP_METHODS  # ... and this project's own multistep methods (transport/multistep.py)


def _unknown_method(method):
    if method in NOT_BUILT_METHODS:
        return NotImplementedError(f"ODE method '{method}' of torchdiffeq is not built here (built: {', '.join(BUILT_METHODS)})")
    return ValueError(f"unknown ODE method '{method}' (torchdiffeq names built here: {', '.join(ALL_METHODS)}; multistep methods: "
                      f"{', '.join(MULTISTEP_METHODS)})")


def _call(func, t, y):
    # torchdiffeq's _PerturbFunc casts the time to the state dtype before calling the user function
    return func(t.to(y.dtype), y)


def fixed_grid_odeint(func, y0, t, method="euler"):
    """Solution of dy/dt = func(t, y) at every point of the grid ``t`` (the grid IS the step sequence).

    Restates torchdiffeq.odeint(..., method in {euler, midpoint, rk4}) with no ``step_size`` option:
    euler    y1 = y0 + dt f(t0, y0)
    midpoint y1 = y0 + dt f(t0 + dt/2, y0 + dt/2 f(t0, y0))
    rk4      3/8-rule variant (rk4_alt_step_func): k2 at t0+dt/3, k3 at t0+2dt/3, k4 at t1, weights 1/8 (1,3,3,1)
    heun2    y1 = y0 + dt/2 (f(t0, y0) + f(t1, y0 + dt f(t0, y0)))                                  [tableau alpha 1 | 1 | 1/2 1/2]
    heun3    k2 at t0+dt/3 (y0 + dt/3 k1), k3 at t0+2dt/3 (y0 + 2dt/3 k2), y1 = y0 + dt (k1 + 3 k3) / 4  [1/3 2/3 | 1/3; 0 2/3 | 1/4 0 3/4]
    """
    if method not in FIXED_GRID_METHODS + HOST_FIXED_GRID_METHODS:
        raise _unknown_method(method)
    out = th.empty((len(t),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
    out[0] = y0
    y = y0
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    for j in range(len(t) - 1):
        t0, t1 = t[j], t[j + 1]
        dt = t1 - t0
        k1 = _call(func, t0, y)
        if method == "euler":
            dy = dt * k1
        elif method == "midpoint":
            half = 0.5 * dt
            dy = dt * _call(func, t0 + half, y + k1 * half)
        elif method == "heun2":
            k2 = _call(func, t1, y + dt * k1)
            dy = dt * (k1 * 0.5 + k2 * 0.5)
        elif method == "heun3":
            k2 = _call(func, t0 + dt * third, y + dt * k1 * third)
            k3 = _call(func, t0 + dt * two_thirds, y + dt * k2 * two_thirds)
            dy = dt * (k1 * 0.25 + k3 * 0.75)
        else:
            k2 = _call(func, t0 + dt * third, y + dt * k1 * third)
            k3 = _call(func, t0 + dt * two_thirds, y + dt * (k2 - k1 * third))
            k4 = _call(func, t1, y + dt * (k1 - k2 + k3))
            dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        y = y + dy
        out[j + 1] = y
    return out


# ---- torchdiffeq's adaptive Dormand-Prince 5(4) (rk_common.RKAdaptiveStepsizeODESolver + dopri5.py) -------------------
_DP_ALPHA = (1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
_DP_BETA = (
    (1 / 5,),
    (3 / 40, 9 / 40),
    (44 / 45, -56 / 15, 32 / 9),
    (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
    (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
    (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84),
)
_DP_C_SOL = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.0)
_DP_C_ERR = (35 / 384 - 1951 / 21600, 0.0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 + 12231 / 42400,
             11 / 84 - 649 / 6300, -1 / 60)
_DP_C_MID = (6025192743 / 30085553152 / 2, 0.0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
             187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2)


# (alpha, beta, c_sol, c_err, c_mid, order) of torchdiffeq's other adaptive Runge-Kutta solvers (bosh3.py, fehlberg2.py, adaptive_heun.py)
_TABLEAUS = {
    "dopri5": (_DP_ALPHA, _DP_BETA, _DP_C_SOL, _DP_C_ERR, _DP_C_MID, 5),
    "bosh3": ((1 / 2, 3 / 4, 1.0), ((1 / 2,), (0.0, 3 / 4), (2 / 9, 1 / 3, 4 / 9)), (2 / 9, 1 / 3, 4 / 9, 0.0),
              (2 / 9 - 7 / 24, 1 / 3 - 1 / 4, 4 / 9 - 1 / 3, -1 / 8), (0.0, 0.5, 0.0, 0.0), 3),
    "fehlberg2": ((1 / 2, 1.0), ((1 / 2,), (1 / 256, 255 / 256)), (1 / 512, 255 / 256, 1 / 512), (-1 / 512, 0.0, 1 / 512), (0.0, 0.5, 0.0), 2),
    "adaptive_heun": ((1.0,), ((1.0,),), (0.5, 0.5), (0.5, -0.5), (0.5, 0.0), 2),
}


def _rms(x):
    return x.float().pow(2).mean().sqrt()


def dopri5_odeint(func, y0, t, **kw):
    """torchdiffeq.odeint(..., method="dopri5") - see adaptive_odeint"""
    return adaptive_odeint(func, y0, t, method="dopri5", **kw)


def adaptive_odeint(func, y0, t, *, method="dopri5", rtol=1e-3, atol=1e-6, max_num_steps=2 ** 31 - 1, stats=None, norm=None, first_step=None):
    """torchdiffeq.odeint(func, y0, t, rtol=rtol, atol=atol, method=...) for the adaptive Runge-Kutta family (rk_common.
    RKAdaptiveStepsizeODESolver): solution at every point of ``t`` (dense output through the quartic fitted to y0, y1, a mid-point
    value and the end slopes), steps chosen by the embedded error estimate.  ``method``: dopri5 (5(4), FSAL), bosh3 (3(2), FSAL),
    fehlberg2 (2(1)), adaptive_heun (2(1)); like torchdiffeq, the last stage's slope stands in for f(t1, y1) also where the tableau is
    not first-same-as-last.

    Follows torchdiffeq's controller: initial step from Hairer's heuristic (``_select_initial_step``), error ratio =
    rms(err / (atol + rtol max(|y0|, |y1|))), accept if <= 1, next step = dt * min(10, max(0.9 ratio^-1/5, 0.2 or 1)).
    ``stats`` (optional dict) receives the number of function evaluations, accepted / rejected steps, the first step size and the
    list of attempted step sizes (``first_step``, ``dt``: Python floats of the fp32 values); ``norm`` replaces the rms norm of the
    controller (tuple states use torchdiffeq's mixed norm, see ``tuple_odeint``); ``first_step`` (torchdiffeq's option of that name)
    is used instead of the heuristic when given - the heuristic's second evaluation is then not made.

    With an engine-backed model callable ``ode.sample`` runs this loop inside the engine instead (``lt_sample_ode_adaptive``)."""
    if method not in _TABLEAUS:
        raise _unknown_method(method)
    ALPHA, BETA, C_SOL, C_ERR, C_MID, order = _TABLEAUS[method]
    fsal = C_SOL[-1] == 0.0 and tuple(C_SOL[:-1]) == tuple(BETA[-1])
    nrm = norm if norm is not None else _rms
    t = t.to(device=y0.device)
    tdt = t.dtype

    def f(tt, y):
        return _call(func, tt.to(tdt) if th.is_tensor(tt) else th.as_tensor(tt, dtype=tdt, device=y0.device), y)

    nfe = 0
    t0 = t[0]
    f0 = f(t0, y0)
    nfe += 1
    if first_step is not None:
        dt = th.as_tensor(first_step, dtype=tdt, device=y0.device)
    else:
        # _select_initial_step(func, t0, y0, order - 1, ...)
        scale = atol + y0.abs() * rtol
        d0, d1 = nrm(y0 / scale), nrm(f0 / scale)
        h0 = 0.01 * d0 / d1 if (float(d0) >= 1e-5 and float(d1) >= 1e-5) else th.tensor(1e-6, device=y0.device)
        h0 = h0.to(tdt)
        f1 = f(t0 + h0, y0 + h0.to(y0.dtype) * f0)
        nfe += 1
        d2 = nrm((f1 - f0) / scale) / h0
        if float(d1) <= 1e-15 and float(d2) <= 1e-15:
            h1 = th.max(th.tensor(1e-6, dtype=tdt, device=y0.device), h0 * 1e-3)
        else:
            h1 = (0.01 / th.max(d1, d2)) ** (1.0 / float(order))
        dt = th.min(100 * h0, h1.to(tdt)).to(tdt)
    dt_first, dts = dt, []

    out = th.empty((len(t),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
    out[0] = y0
    y, fy, tcur = y0, f0, t0
    tprev = t0
    coeffs = [y0] * 5
    accepted = rejected = 0
    for i in range(1, len(t)):
        next_t = t[i]
        steps = 0
        while float(next_t) > float(tcur):
            assert steps < max_num_steps, "max_num_steps exceeded"
            steps += 1
            if stats is not None:
                dts.append(dt)
            t1 = tcur + dt
            dty = dt.to(y.dtype)
            k = [fy]
            yi = y
            for alpha, beta in zip(ALPHA, BETA):
                ti = t1 if alpha == 1.0 else tcur + alpha * dt
                acc = k[0] * beta[0]
                for kj, bj in zip(k[1:], beta[1:]):
                    if bj != 0.0:
                        acc = acc + kj * bj
                yi = y + dty * acc
                k.append(f(ti, yi))
                nfe += 1
            f_1 = k[-1]
            if fsal:  # the last stage IS the solution (dopri5, bosh3)
                y1 = yi
            else:
                sol = k[0] * C_SOL[0]
                for kj, cj in zip(k[1:], C_SOL[1:]):
                    if cj != 0.0:
                        sol = sol + kj * cj
                y1 = y + dty * sol
            err = k[0] * C_ERR[0]
            for kj, cj in zip(k[1:], C_ERR[1:]):
                if cj != 0.0:
                    err = err + kj * cj
            err = dty * err
            tol = atol + rtol * th.max(y.abs(), y1.abs())
            ratio = float(nrm(err / tol))
            if ratio <= 1.0:  # accept: dense-output coefficients of this step, then move on
                mid = k[0] * C_MID[0]
                for kj, cj in zip(k[1:], C_MID[1:]):
                    if cj != 0.0:
                        mid = mid + kj * cj
                y_mid = y + dty * mid
                a = 2 * dty * (f_1 - fy) - 8 * (y1 + y) + 16 * y_mid
                b = dty * (5 * fy - 3 * f_1) + 18 * y + 14 * y1 - 32 * y_mid
                c = dty * (f_1 - 4 * fy) - 11 * y - 5 * y1 + 16 * y_mid
                coeffs = [y, dty * fy, c, b, a]
                tprev, tcur, y, fy = tcur, t1, y1, f_1
                accepted += 1
            else:
                rejected += 1
            # _optimal_step_size(dt, ratio, safety 0.9, ifactor 10, dfactor 0.2, order)
            if ratio == 0.0:
                dt = dt * 10.0
            else:
                dfactor = 1.0 if ratio < 1.0 else 0.2
                dt = dt * min(10.0, max(0.9 / ratio ** (1.0 / order), dfactor))
        # _interp_evaluate(coeffs, tprev, tcur, next_t)
        x = ((next_t - tprev) / (tcur - tprev)).to(y.dtype)
        total = coeffs[0] + x * coeffs[1]
        xp = x
        for cf in coeffs[2:]:
            xp = xp * x
            total = total + xp * cf
        out[i] = total
    if stats is not None:
        stats.update(nfe=nfe, accepted=accepted, rejected=rejected, first_step=float(dt_first),
                     dt=th.stack(dts).tolist() if dts else [])
    return out


def tuple_odeint(func, y0, t, *, method, rtol=1e-3, atol=1e-6):
    """torchdiffeq.odeint on a TUPLE state (the likelihood ODE's (x, delta_logp), reference transport.py:431-433): the tuple is
    flattened into one 1-d state (``_check_inputs``: cat of reshape(-1)), the user function wrapped (``_TupleFunc``), the solution
    split back into a tuple of [len(t), *shape] tensors; the adaptive controller then measures with the MIXED norm = max over the
    components of their rms norms (``_mixed_norm``).  One tolerance for all components (the reference passes [atol] * len(x))."""
    shapes = [tuple(y.shape) for y in y0]
    sizes = [y.numel() for y in y0]

    def split(flat, lead=()):
        out, o = [], 0
        for sh, n in zip(shapes, sizes):
            out.append(flat[..., o:o + n].reshape(lead + sh))
            o += n
        return tuple(out)

    def f(tt, flat):
        return th.cat([g.reshape(-1) for g in func(tt, split(flat))])

    def mixed_norm(flat):
        return th.stack([_rms(c) for c in split(flat)]).max()

    flat0 = th.cat([y.reshape(-1) for y in y0])
    if method in ADAPTIVE_METHODS:
        sol = adaptive_odeint(f, flat0, t, method=method, rtol=rtol, atol=atol, norm=mixed_norm)
    else:
        sol = fixed_grid_odeint(f, flat0, t, method=method)
    return split(sol, (len(t),))


def _engine_target(model):
    """(NextDiT instance, use_cfg) when ``model`` is one of our engine-backed bound methods, else None."""
    owner = getattr(model, "__self__", None)
    name = getattr(model, "__name__", "")
    if owner is None or not hasattr(owner, "_engine_sample_ode"):
        return None
    if name == "forward_with_cfg":
        return owner, True
    if name == "forward":
        return owner, False
    return None


class ode:
    """ODE solver front end (reference integrators.py:79-116)."""

    def __init__(self, drift, *, t0, t1, sampler_type, num_steps, atol, rtol, time_shifting_factor=None):
        assert t0 < t1, "ODE sampler has to be in forward time"
        self.drift = drift
        self.t = th.linspace(t0, t1, num_steps)
        if time_shifting_factor:
            s = time_shifting_factor
            self.t = self.t / (self.t + s - s * self.t)
        self.atol, self.rtol = atol, rtol
        self.sampler_type = sampler_type
        # torchdiffeq >= 0.2 casts t to the state dtype inside its function wrapper; keep switchable
        self.t_round_to_state_dtype = True
        self.use_engine = True    # adaptive and multistep methods: False keeps the host loop (adaptive_odeint) for an engine-backed callable too
        self.first_step = None    # adaptive methods: torchdiffeq's option of that name (None: the initial-step heuristic)
        self.max_num_steps = 2 ** 31 - 1
        self.stats = None         # adaptive methods: nfe / accepted / rejected / first_step / dt of the last sample() call

    def _sample_cfg_schedule(self, x, model, table, model_kwargs, rescale=0.0, norm_limit=math.inf, reuse=None, slg=None, slg_layers=(), pag=None, pag_layers=()):
        """a guidance schedule (transport/guidance.py): one engine call for an engine-backed forward_with_cfg, else the host loop"""
        from .guidance import (cfg_table, refuse_rule_with_reuse, rule_is_off, sample_cfg_multistep, sample_cfg_reuse, sample_cfg_reuse_multistep,
                               sample_cfg_rule, sample_cfg_schedule)
        if (isinstance(x, tuple) or not getattr(self.drift, "is_plain_velocity", False)
                or self.sampler_type not in FIXED_GRID_METHODS + MULTISTEP_METHODS):
            raise NotImplementedError("guidance schedules are built for the fixed-grid methods on a tensor state with the plain velocity as drift")
        rule_off = rule_is_off(rescale, norm_limit)
        if table is None:  # a rule without a table: one scale for every stage
            table = cfg_table(self.t, self.sampler_type, model_kwargs.get("cfg_scale", 1.0))
        if reuse is not None:  # guidance reuse: refused together with a rule and on a packed list, by name
            if isinstance(x, (list, tuple)):
                raise ValueError("guidance reuse (cfg_reuse) takes a tensor state; a packed batch (a list of latents) is not served")
            refuse_rule_with_reuse(rescale, norm_limit)
        if slg is not None:  # skip-layer guidance: refused by name on a packed list, with a rule, a reuse table, another method
            from .guidance import refuse_with_slg, sample_cfg_slg
            if isinstance(x, (list, tuple)):
                raise ValueError("skip-layer guidance (slg_table) takes a tensor state; a packed batch (a list of latents) is not served")
            refuse_with_slg(slg, self.sampler_type, rescale, norm_limit, reuse)
        if pag is not None:  # perturbed-attention guidance: refused by name with what skip-layer guidance refuses, and with an slg table
            from .guidance import refuse_with_pag, sample_cfg_pag
            if isinstance(x, (list, tuple)):
                raise ValueError("perturbed-attention guidance (pag_table) takes a tensor state; a packed batch (a list of latents) is not served")
            refuse_with_pag(pag, self.sampler_type, rescale, norm_limit, reuse, slg)
        target = _engine_target(model)
        if target is not None and target[1] and x.is_cuda and self.use_engine and hasattr(target[0], "_engine_sample_ode_cfg_schedule"):
            if pag is not None:
                return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs),
                                                                 pag=pag, pag_layers=pag_layers, slg_layers=slg_layers)
            if slg is not None:
                return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs),
                                                                 slg=slg, slg_layers=slg_layers)
            if reuse is not None:
                return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs),
                                                                 reuse=reuse)
            if rule_off:  # the call it was before the rule existed
                return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs))
            return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs),
                                                             rescale=rescale, norm_limit=norm_limit)
        owner = getattr(model, "__self__", None)
        if owner is None or getattr(model, "__name__", "") != "forward_with_cfg" or not hasattr(owner, "forward"):
            raise TypeError("cfg_table needs the bound forward_with_cfg of a model that also has forward (the conditional-only stages call it)")
        if pag is not None:
            return sample_cfg_pag(owner, x, self.t, table, pag, pag_layers, slg_layers, self.sampler_type, t_round=self.t_round_to_state_dtype,
                                  **model_kwargs)
        if slg is not None:
            return sample_cfg_slg(owner, x, self.t, table, slg, slg_layers, self.sampler_type, t_round=self.t_round_to_state_dtype, **model_kwargs)
        if reuse is not None and self.sampler_type in MULTISTEP_METHODS:
            return sample_cfg_reuse_multistep(owner, x, self.t, table, reuse, self.sampler_type, t_round=self.t_round_to_state_dtype, **model_kwargs)
        if reuse is not None:
            return sample_cfg_reuse(owner, x, self.t, table, reuse, self.sampler_type, t_round=self.t_round_to_state_dtype, **model_kwargs)
        if self.sampler_type in MULTISTEP_METHODS:
            return sample_cfg_multistep(owner, x, self.t, table, self.sampler_type, rescale=rescale, norm_limit=norm_limit,
                                        t_round=self.t_round_to_state_dtype, **model_kwargs)
        if rule_off:
            return sample_cfg_schedule(owner, x, self.t, table, self.sampler_type, t_round=self.t_round_to_state_dtype, **model_kwargs)
        return sample_cfg_rule(owner, x, self.t, table, self.sampler_type, rescale=rescale, norm_limit=norm_limit,
                               t_round=self.t_round_to_state_dtype, **model_kwargs)

    def _sample_teacache(self, x, model, threshold, coefficients, model_kwargs, **others):
        """step caching (transport/cache.py): one engine call for an engine-backed forward / forward_with_cfg; everything else is
        refused by name - the host loop needs the probe, which only the engine offers"""
        from .cache import IDENTITY, check_cache_args, refuse_with_teacache
        refuse_with_teacache(self.sampler_type, packed=isinstance(x, (list, tuple)), **others)
        check_cache_args(threshold, IDENTITY if coefficients is None else coefficients)
        target = _engine_target(model)
        if target is None or not hasattr(target[0], "_engine_sample_ode_teacache"):
            raise TypeError("step caching (teacache) needs the bound forward / forward_with_cfg of an engine-backed model: the rule probes the "
                            "head of every evaluation, which only the engine offers")
        if not getattr(self.drift, "is_plain_velocity", False):
            raise NotImplementedError("step caching (teacache) is built for the plain velocity as drift")
        owner, use_cfg = target
        return owner._engine_sample_ode_teacache(x, self.t, self.sampler_type, use_cfg, self.t_round_to_state_dtype, dict(model_kwargs), threshold,
                                                 IDENTITY if coefficients is None else coefficients)

    def sample(self, x, model, cfg_table=None, cfg_rescale=0.0, cfg_norm_limit=math.inf, cfg_reuse=None, slg_table=None, slg_layers=(),
               teacache=None, teacache_coefficients=None, pag_table=None, pag_layers=(), cfg_apg=None, cfg_zero_star=False, cfg_zero_init=0,
               windows=None, window_weights=None, compose=None, seg_table=None, seg_layers=(), seg_sigma=None, **model_kwargs):
        if seg_table is not None:  # smoothed-energy guidance (transport/guidance.py): its refusals come first, by name; None: the call it was
            from .guidance import sample_seg_front
            if isinstance(x, tuple) or not getattr(self.drift, "is_plain_velocity", False):
                raise NotImplementedError("smoothed-energy guidance is built for a tensor state with the plain velocity as drift")
            return sample_seg_front(x, model, self.t, self.sampler_type, cfg_table, model_kwargs, seg_table, seg_layers, seg_sigma, slg_layers,
                                    t_round=self.t_round_to_state_dtype, use_engine=self.use_engine,
                                    project=True if (cfg_apg is not None or cfg_zero_star or cfg_zero_init) else None, compose=compose,
                                    windows=windows, rescale=cfg_rescale, norm_limit=cfg_norm_limit, reuse=cfg_reuse, slg=slg_table,
                                    teacache=teacache, pag=pag_table)
        if compose is not None:  # composed guidance (transport/guidance.py): its refusals come first, by name
            from .guidance import sample_compose_front
            if isinstance(x, tuple) or not getattr(self.drift, "is_plain_velocity", False):
                raise NotImplementedError("composed guidance is built for a tensor state with the plain velocity as drift")
            return sample_compose_front(x, model, self.t, self.sampler_type, model_kwargs, compose, t_round=self.t_round_to_state_dtype,
                                        use_engine=self.use_engine, cfg_table=cfg_table,
                                        rule=None if (float(cfg_rescale) == 0.0 and float(cfg_norm_limit) == math.inf) else True,
                                        cfg_reuse=cfg_reuse, slg=slg_table, pag=pag_table,
                                        project=True if (cfg_apg is not None or cfg_zero_star or cfg_zero_init) else None, teacache=teacache,
                                        windows=windows)
        if windows is not None:  # tiled (MultiDiffusion) sampling (transport/tiled.py): its refusals come first, by name
            from .tiled import sample_tiled_front
            if isinstance(x, tuple) or not getattr(self.drift, "is_plain_velocity", False):
                raise NotImplementedError("tiled sampling is built for a tensor state with the plain velocity as drift")
            return sample_tiled_front(x, model, self.t, self.sampler_type, model_kwargs, windows, window_weights,
                                      t_round=self.t_round_to_state_dtype, use_engine=self.use_engine, cfg_table=cfg_table,
                                      rule=None if (float(cfg_rescale) == 0.0 and float(cfg_norm_limit) == math.inf) else True,
                                      cfg_reuse=cfg_reuse, slg=slg_table, pag=pag_table,
                                      project=True if (cfg_apg is not None or cfg_zero_star or cfg_zero_init) else None, teacache=teacache)
        if window_weights is not None:
            raise ValueError("window_weights belongs to tiled sampling: pass windows=(offsets, (win_h, win_w)) too")
        if cfg_apg is not None or cfg_zero_star or cfg_zero_init:  # projected guidance: its refusals come first, by name
            from .guidance import sample_project_front
            if not getattr(self.drift, "is_plain_velocity", False):
                raise NotImplementedError("projected guidance is built for the plain velocity as drift")
            return sample_project_front(x, model, self.t, self.sampler_type, cfg_table, model_kwargs, apg=cfg_apg, zero_star=cfg_zero_star,
                                        zero_init=cfg_zero_init, t_round=self.t_round_to_state_dtype, use_engine=self.use_engine,
                                        rescale=cfg_rescale, norm_limit=cfg_norm_limit, reuse=cfg_reuse, slg=slg_table, pag=pag_table,
                                        teacache=teacache)
        if pag_table is not None:  # perturbed-attention guidance: its refusals come first, by name
            from .guidance import refuse_with_pag
            refuse_with_pag(pag_table, self.sampler_type, cfg_rescale, cfg_norm_limit, cfg_reuse, slg_table, teacache)
            return self._sample_cfg_schedule(x, model, cfg_table, model_kwargs, cfg_rescale, cfg_norm_limit, cfg_reuse, None, slg_layers,
                                             pag_table, pag_layers)
        if teacache is not None:  # (None: the call made without it)
            return self._sample_teacache(x, model, teacache, teacache_coefficients, model_kwargs, cfg_table=cfg_table, cfg_rescale=cfg_rescale,
                                         cfg_norm_limit=cfg_norm_limit, cfg_reuse=cfg_reuse, slg=slg_table)
        if (cfg_table is not None or cfg_reuse is not None or slg_table is not None
                or not (float(cfg_rescale) == 0.0 and float(cfg_norm_limit) == math.inf)):
            return self._sample_cfg_schedule(x, model, cfg_table, model_kwargs, cfg_rescale, cfg_norm_limit, cfg_reuse, slg_table, slg_layers)
        if isinstance(x, tuple):  # the likelihood ODE (reference integrators.py:105-115 with a tuple state)
            device = x[0].device

            def _fn_tuple(t, y):
                return self.drift(y, th.ones(y[0].size(0)).to(device) * t, model, **model_kwargs)

            if self.sampler_type in MULTISTEP_METHODS:
                raise NotImplementedError(f"the multistep method '{self.sampler_type}' is built for tensor states (the likelihood ODE runs the "
                                          "Runge-Kutta methods)")
            return tuple_odeint(_fn_tuple, x, self.t.to(device), method=self.sampler_type, rtol=self.rtol, atol=self.atol)
        target = _engine_target(model)
        if (target is not None and getattr(self.drift, "is_plain_velocity", False) and x.is_cuda and self.use_engine
                and x.dtype in (th.float32, th.bfloat16) and self.sampler_type in MULTISTEP_METHODS and len(self.t) >= 2
                and hasattr(target[0], "_engine_sample_ode_multistep")):
            owner, use_cfg = target
            return owner._engine_sample_ode_multistep(x, self.t, self.sampler_type, use_cfg, self.t_round_to_state_dtype, dict(model_kwargs))
        if (target is not None and getattr(self.drift, "is_plain_velocity", False) and x.is_cuda
                and self.sampler_type in FIXED_GRID_METHODS):
            return self._sample_on_engine(x, target, model_kwargs)
        if (target is not None and getattr(self.drift, "is_plain_velocity", False) and x.is_cuda and self.use_engine
                and x.dtype in (th.float32, th.bfloat16) and self.sampler_type in ADAPTIVE_METHODS
                and hasattr(target[0], "_engine_sample_ode_adaptive")):
            owner, use_cfg = target
            out, self.stats = owner._engine_sample_ode_adaptive(
                x, self.t, self.sampler_type, use_cfg, self.t_round_to_state_dtype, dict(model_kwargs), rtol=self.rtol, atol=self.atol,
                first_step=self.first_step, max_steps=self.max_num_steps)
            return out

        device = x.device

        def _fn(t, y):
            tvec = th.ones(y.size(0)).to(device) * t  # fp32 [B] (reference integrators.py:108)
            return self.drift(y, tvec, model, **model_kwargs)

        if self.sampler_type in MULTISTEP_METHODS:
            return multistep_odeint(_fn, x, self.t.to(device), self.sampler_type, t_round=self.t_round_to_state_dtype)
        if self.sampler_type in ADAPTIVE_METHODS:
            self.stats = {}
            return adaptive_odeint(_fn, x, self.t.to(device), method=self.sampler_type, rtol=self.rtol, atol=self.atol,
                                   first_step=self.first_step, max_num_steps=self.max_num_steps, stats=self.stats)
        return fixed_grid_odeint(_fn, x, self.t.to(device), method=self.sampler_type)

    def _sample_on_engine(self, x, target, kw):
        """whole trajectory in one C-ABI call (lt_sample_ode): the model class maps its own forward / forward_with_cfg
        kwargs onto the engine (each reference sub-project has a different kwarg set)"""
        owner, use_cfg = target
        return owner._engine_sample_ode(x, self.t, self.sampler_type, use_cfg, self.t_round_to_state_dtype, dict(kw))


_SDE_TENSOR_FORMS = ("SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing")  # "constant" yields a Python float (fails in th.sqrt)


def sde_table(plan, form, norm, t, dt, sampler_type, like, last_step=None, last_step_size=0.0, t1=None):
    """Per-stage scalar coefficients of the SDE loop for ``lt_sample_sde``: every row of the batch carries the same t, so the
    ``[B,1,1,1]`` tensors the path plan produces inside ``sde_drift`` are one value per stage.  They are computed HERE by the plan's own
    functions on tensors of the state's dtype on the state's device (``like``), one row per step instead of one row per sample - the
    same elementwise torch kernels the host loop runs, so the rounding is torch's, not a re-derivation - and read back once.

    Returns ``(steps, last)``: ``steps`` fp32 CPU ``[(len(t) - 1) * stages, 8]`` with records ``t, r, var, D, q, dt, sqrt_dt, hdt``
    (stages = 2 for Heun: the stage at t, then the stage at t + dt), ``last`` fp32 CPU ``[8]`` = ``t, r, var, D, h, a, c, 0`` at the fp32
    time ``t1`` (None without a last step).  r = alpha / alpha', var = sigma^2 - r sigma' sigma (``get_score_from_velocity``), D the
    diffusion coefficient, q = sqrt(2 D); dt, sqrt_dt and hdt = 0.5 dt are the fp32 values of the loop's 0-dim CPU tensors, which
    PyTorch multiplies with a device tensor in fp32 whatever its dtype (they are NOT rounded to the state dtype)."""
    dev, dtype = like.device, like.dtype
    n = len(t) - 1
    stages = 2 if sampler_type == "Heun" else 1

    def coeffs(tvec, xl):
        r, sigma_t, d_sigma_t = plan._ratio_and_coeffs(xl, tvec)
        var = sigma_t**2 - r * d_sigma_t * sigma_t  # the denominator of ICPlan.get_score_from_velocity, same expression
        D = plan.compute_diffusion(xl, tvec, form=form, norm=norm)
        return [v.reshape(-1).float() for v in (r, var, D, th.sqrt(2 * D))]

    with th.no_grad():
        xl = th.zeros((n, 1, 1, 1), dtype=dtype, device=dev)
        tvec = t[:-1].to(dev).to(dtype)  # th.ones(B).to(x) * t of the loop: the fp32 grid value rounded to the state dtype
        rows = []
        for k in range(stages):
            tk = tvec if k == 0 else tvec + dt  # _heun: tvec + self.dt (state-dtype tensor + 0-dim CPU fp32 tensor)
            rows.append(th.stack([tk.float()] + coeffs(tk, xl), dim=1))
        last = None
        if last_step is not None:
            ts = th.ones(1, device=dev) * t1  # fp32, as Sampler.sample_sde builds it
            r, var, D, _ = coeffs(ts, xl[:1])
            a = plan.compute_alpha_t(ts)[0][0]
            sg = plan.compute_sigma_t(ts)[0][0]
            h = th.tensor([last_step_size], dtype=th.float32, device=dev)
            last = th.cat([ts, r, var, D, h, a.to(dtype).float().reshape(1), ((sg**2) / a).reshape(1), th.zeros(1, device=dev)])
        dev_rows = th.stack(rows, dim=1).reshape(n * stages, 5)  # step-major: stage 0, stage 1 of step 0, ...
        packed = th.cat([dev_rows.reshape(-1)] + ([last] if last is not None else [])).cpu()  # the ONE read-back
    steps = th.empty((n * stages, 8), dtype=th.float32)
    steps[:, :5] = packed[: n * stages * 5].reshape(n * stages, 5)
    steps[:, 5] = float(dt)
    steps[:, 6] = float(th.sqrt(dt))
    steps[:, 7] = float(0.5 * dt)
    return steps, (packed[n * stages * 5:].clone() if last is not None else None)


def views_guided_table(tgrid, state_dtype, coef_rounding="fp32"):
    """Per-stage scalar coefficients of ``lt_sample_views_guided`` (Phase Upscale of the reference's visual_anagrams/generate.py:232-257): fp32
    CPU ``[len(tgrid) - 1, 2, 4]`` with records ``ft, f1t, kc, k1c`` for the stage at ``t0`` and the stage at ``t_mid = t0 + 0.5 (t1 - t0)``.

    ``ft = fp32(t)``, ``f1t = fp32(1 - t)``: ``t0 * guidance`` and ``(1 - t0) * noise`` have a Python float on the left, which PyTorch multiplies
    into a tensor in fp32 whatever its dtype.  ``kc = c`` and ``k1c = 1 - c`` with ``c = 0.5 * (1 + torch.cos(torch.pi * torch.tensor(t)))``, the
    reference's own expression evaluated here by torch: a 0-dim fp32 CPU tensor.  ``coef_rounding="state"`` rounds ``c`` and ``1 - c`` to
    ``state_dtype`` before the upload - what PyTorch's CPU kernels do with a 0-dim operand of a bf16 tensor; ``"fp32"`` keeps them, which is what
    its GPU kernels are expected to do with a CPU scalar."""
    if coef_rounding not in ("fp32", "state"):
        raise ValueError(f"coef_rounding '{coef_rounding}' not in ('fp32', 'state')")
    t = tgrid if isinstance(tgrid, th.Tensor) else th.tensor(list(tgrid), dtype=th.float32)
    grid = [float(v) for v in t.detach().to("cpu", th.float32).tolist()]  # the fp32 grid's values as Python floats (generate.py:385)
    out = th.empty((max(len(grid) - 1, 0), 2, 4), dtype=th.float32)
    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = t1 - t0
        half_dt = 0.5 * dt
        for k, tk in enumerate((t0, t0 + half_dt)):
            c = 0.5 * (1 + th.cos(th.pi * th.tensor(tk)))
            k1c = 1 - c
            if coef_rounding == "state":
                c, k1c = c.to(state_dtype).float(), k1c.to(state_dtype).float()
            out[i, k] = th.stack([th.tensor(tk, dtype=th.float32), th.tensor(1 - tk, dtype=th.float32), c.float(), k1c.float()])
    return out


class sde:
    """Euler-Maruyama / Heun SDE sampler (reference integrators.py:5-76).

    With an engine-backed model callable, velocity prediction, a state on the GPU and a diffusion form that yields tensors the whole
    trajectory - and, through ``sample_with_last_step``, the last-step rule - runs inside the C-ABI engine (``lt_sample_sde``: one host
    loop in C++, ONE model evaluation per stage instead of the two of ``drift + diffusion * score``, the noise uploaded once).  Anything
    else (another callable, score / noise prediction, a CPU state, the ``"constant"`` form) runs the reference's loop below through the
    model callable, unchanged.  ``use_engine = False`` switches back to that loop."""

    def __init__(self, drift, diffusion, *, t0, t1, num_steps, sampler_type, engine_plan=None, finish=None):
        assert t0 < t1, "SDE sampler has to be in forward time"
        self.num_timesteps = num_steps
        self.t = th.linspace(t0, t1, num_steps)
        self.dt = self.t[1] - self.t[0]
        self.drift, self.diffusion = drift, diffusion
        if sampler_type not in ("Euler", "Heun"):
            raise NotImplementedError("Smapler type not implemented.")
        self.sampler_type = sampler_type
        # what Sampler.sample_sde knows and the engine path needs: dict(plan, form, norm, velocity, last_step, last_step_size, t1)
        self.engine_plan = engine_plan
        self.finish = finish
        self.use_engine = True

    def _euler_maruyama(self, x, mean_x, t, model, **kw):
        noise = th.randn(x.size()).to(x)
        tvec = th.ones(x.size(0)).to(x) * t
        dw = noise * th.sqrt(self.dt)
        mean_x = x + self.drift(x, tvec, model, **kw) * self.dt
        return mean_x + th.sqrt(2 * self.diffusion(x, tvec)) * dw, mean_x

    def _heun(self, x, _, t, model, **kw):
        noise = th.randn(x.size()).to(x)
        dw = noise * th.sqrt(self.dt)
        tvec = th.ones(x.size(0)).to(x) * t
        xhat = x + th.sqrt(2 * self.diffusion(x, tvec)) * dw
        k1 = self.drift(xhat, tvec, model, **kw)
        k2 = self.drift(xhat + self.dt * k1, tvec + self.dt, model, **kw)
        return xhat + 0.5 * self.dt * (k1 + k2), xhat

    def _engine_target(self, init, model):
        ep = self.engine_plan
        if not self.use_engine or ep is None or not ep["velocity"] or ep["form"] not in _SDE_TENSOR_FORMS:
            return None
        if not th.is_tensor(init) or not init.is_cuda or init.dtype not in (th.float32, th.bfloat16) or len(self.t) < 2:
            return None
        target = _engine_target(model)
        return target if target is not None and hasattr(target[0], "_engine_sample_sde") else None

    def _sample_on_engine(self, init, target, kw, with_last):
        """the loop (and the last step) in one C-ABI call; the noise is drawn exactly as the loop draws it - one th.randn(x.size()) per
        step from torch's CPU generator, in step order - into one pinned buffer that is uploaded once"""
        owner, use_cfg = target
        ep = self.engine_plan
        last_step = ep["last_step"] if with_last else None
        n = len(self.t) - 1
        with th.no_grad():
            steps, last = sde_table(ep["plan"], ep["form"], ep["norm"], self.t, self.dt, self.sampler_type, init, last_step,
                                    ep["last_step_size"], ep["t1"])
            draws = th.empty((n,) + tuple(init.shape), dtype=th.float32, pin_memory=True)
            for i in range(n):
                draws[i] = th.randn(init.size())
            noise = draws.to(init.device, non_blocking=True).to(init.dtype)
            _, traj, final = owner._engine_sample_sde(init, noise, steps, last, self.sampler_type, last_step, use_cfg, dict(kw))
        xs = list(traj.unbind(0))
        if with_last:
            xs.append(final if final is not None else xs[-1])
        return xs

    def sample(self, init, model, **model_kwargs):
        target = self._engine_target(init, model)
        if target is not None:
            return self._sample_on_engine(init, target, model_kwargs, with_last=False)
        step = self._euler_maruyama if self.sampler_type == "Euler" else self._heun
        x = mean_x = init
        samples = []
        with th.no_grad():
            for ti in self.t[:-1]:
                x, mean_x = step(x, mean_x, ti, model, **model_kwargs)
                samples.append(x)
        return samples

    def sample_with_last_step(self, init, model, **model_kwargs):
        """``sample`` followed by the last-step rule ``finish`` at t1 (Sampler.sample_sde, reference transport.py:331-342): the list of
        ``num_steps`` states"""
        target = self._engine_target(init, model)
        if target is not None:
            return self._sample_on_engine(init, target, model_kwargs, with_last=True)
        xs = self.sample(init, model, **model_kwargs)
        ts = th.ones(init.size(0), device=init.device) * self.engine_plan["t1"]
        xs.append(self.finish(xs[-1], ts, model, **model_kwargs))
        return xs
