"""Linear multistep ODE samplers on a fixed grid: Adams-Bashforth predictors ``ab2`` / ``ab3`` and predictor-corrector pairs ``abm2`` /
``abm3`` whose corrector costs no model evaluation.  Order 2-3 at ONE evaluation per grid interval, where the one-step solvers
(``midpoint``, ``rk4``) pay 2 or 4.

Grid ``t_0 .. t_N`` (the fp32 grid's values as Python floats), ``f_i = model(x_i, t_i)`` with ``x_i`` the state handed to evaluation ``i``, ``q``
newest slopes kept (2 for ``ab2`` / ``abm2``, 3 for ``ab3`` / ``abm3``)::

    p_0 = y_0 = z
    for i = 0 .. N-1:
        f_i     = model(p_i, t_i)                                        # exactly N evaluations, none at t_N
        y_i     = y_{i-1} + sum_j a_{i,j} f_{i-j}   (abm*, i >= 1)       # corrector; otherwise y_i = p_i
        p_{i+1} = y_i + sum_j b_{i,j} f_{i-j}                            # predictor, from the STORED y_i
    result p_N; recorded state i is y_i for i < N and p_N for i = N

    b_{i,j} = integral over [t_i, t_{i+1}] of L_j,  L_j the Lagrange basis on t_i, t_{i-1}, .., t_{i-m+1},  m  = min(q, i + 1)
    a_{i,j} = integral over [t_{i-1}, t_i] of L_j,  L_j the Lagrange basis on t_i, t_{i-1}, .., t_{i-m'},   m' = min(q, i)

The order ramps up: step 0 is Euler, the corrector of step 1 is the trapezoid rule.  The slope ``f_i`` was evaluated at the PREDICTED state and
is reused as the newest slope of the next predictor - that reuse is why the corrector is free.  The grids here are time-shifted, so the weights
are the variable-step ones; on a uniform grid they are the textbook ``h (3, -1) / 2``, ``h (23, -16, 5) / 12``, ``h (5, 8, -1) / 12``.  These are
not torchdiffeq's ``explicit_adams`` / ``implicit_adams`` (fixed step, order 4 by default, an implicit solve): those names stay refused.

``multistep_table`` computes the weights in float64 by closed-form polynomial integration and rounds them once to fp32: row ``i`` is
``a_{i,0..3}, b_{i,0..3}``, unused entries 0.  The table IS the contract between this loop and the engine (``lt_sample_ode_multistep`` does no
coefficient maths): a weight sum runs over the entries of its row up to the last one that is not 0.  Rounding chain, ``R`` = round to the state
dtype (identity at fp32), a Python-float weight entering torch's op-math as fp32::

    acc = R(c_0 k_0);  acc = R(acc + R(c_j k_j)) for j >= 1;  out = R(y + acc)

``multistep_odeint`` below IS that text in plain torch ops, as ``transport/masked.py`` is for inpainting: it defines the feature, runs callables
that are not engine-backed and CPU states, and is what the engine call is held to, state for state.  Masked (inpainting) sampling with a
multistep method is refused: the blend makes the state discontinuous, so the history's slopes no longer belong to it."""
from __future__ import annotations

import torch as th

MULTISTEP_METHODS = ("ab2", "ab3", "abm2", "abm3")
_SLOPES = {"ab2": 2, "ab3": 3, "abm2": 2, "abm3": 3}  # q
_CORRECTOR = {"ab2": False, "ab3": False, "abm2": True, "abm3": True}

MASKED_REFUSAL = ("masked (inpainting) sampling with a multistep method ({}) is refused: the blend makes the state discontinuous, so the "
                  "history's slopes no longer belong to it - use euler, midpoint or rk4")


def is_corrector(method):
    _check(method)
    return _CORRECTOR[method]


def _check(method):
    if method not in MULTISTEP_METHODS:
        raise ValueError(f"unknown multistep method '{method}' (built: {', '.join(MULTISTEP_METHODS)})")


def _grid_floats(tgrid):
    """the fp32 grid's values as Python floats"""
    t = tgrid if isinstance(tgrid, th.Tensor) else th.tensor(list(tgrid), dtype=th.float32)
    t = t.detach().to("cpu", th.float32)
    if t.dim() != 1 or len(t) < 2:
        raise ValueError("a multistep sampler needs a 1-D grid of at least 2 points")
    return [float(v) for v in t.tolist()]


def _poly_mul(p, q):
    out = [0.0] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            out[i + j] += a * b
    return out


def lagrange_weights(nodes, lo, hi):
    """``[integral over [lo, hi] of L_j]`` for the Lagrange basis on ``nodes``, in float64: each ``L_j`` is expanded in powers of ``s = t - nodes[0]``
    (which keeps the coefficients small) and its antiderivative evaluated at both ends"""
    x0 = nodes[0]
    xs = [x - x0 for x in nodes]
    lo, hi = lo - x0, hi - x0
    out = []
    for j, xj in enumerate(xs):
        poly, den = [1.0], 1.0
        for k, xk in enumerate(xs):
            if k != j:
                poly = _poly_mul(poly, [-xk, 1.0])
                den *= xj - xk
        val = 0.0
        for p, c in enumerate(poly):
            val += c * (hi ** (p + 1) - lo ** (p + 1)) / (p + 1)
        out.append(val / den)
    return out


def _weights(t, method):
    q = _SLOPES[method]
    rows = []
    for i in range(len(t) - 1):
        m = min(q, i + 1)
        b = lagrange_weights([t[i - j] for j in range(m)], t[i], t[i + 1])
        a = []
        if _CORRECTOR[method] and i >= 1:
            a = lagrange_weights([t[i - j] for j in range(min(q, i) + 1)], t[i - 1], t[i])
        rows.append((a + [0.0] * (4 - len(a)), b + [0.0] * (4 - len(b))))
    return rows


def multistep_weights(tgrid, method):
    """the float64 weights before their one rounding: ``(a[4], b[4])`` per interval, zeros where no slope is used"""
    _check(method)
    return _weights(_grid_floats(tgrid), method)


def multistep_table(tgrid, method):
    """fp32 CPU ``[N, 8]``: row ``i`` holds ``a_{i,0..3}, b_{i,0..3}`` (``j`` = 0 the newest slope), unused entries 0"""
    tab = th.tensor([a + b for a, b in multistep_weights(tgrid, method)], dtype=th.float64).to(th.float32)
    if not bool(th.isfinite(tab).all()):
        raise ValueError("multistep table has an entry that is not finite (two grid points coincide?)")
    return tab


def used(c):
    """how many entries of a row's weight sum run: up to the last one that is not 0 (the rule the engine reads the table by)"""
    n = 0
    for j, v in enumerate(c):
        if v != 0.0:
            n = j + 1
    return n


def weight_sum(y, k, c):
    """``y + sum_j c[j] k[j]`` over the used entries of ``c``, rounding as the chain in the module docstring; ``y`` itself where none is used"""
    n = used(c)
    if n == 0:
        return y
    inc = k[0] * c[0]
    for j in range(1, n):
        inc = inc + k[j] * c[j]
    return y + inc


def multistep_odeint(func, y0, t, method, table=None, t_round=True):
    """Every recorded state ``[len(t), *y0.shape]`` of the loop in the module docstring.  ``func(t_i, y)`` is called as ``fixed_grid_odeint`` calls
    it: the time a 0-dim tensor of the grid's dtype on the state's device, cast to the state dtype first (torchdiffeq's rule; ``t_round=False`` hands it over as it is).  ``table``: the
    weights to use instead of ``multistep_table(t, method)`` (an fp32 ``[N, 8]`` tensor; a float64 state takes the float64 weights otherwise)."""
    _check(method)
    grid = t if isinstance(t, th.Tensor) else th.tensor(list(t), dtype=th.float32)
    n = len(grid) - 1
    if table is not None:
        rows = [(r[:4], r[4:]) for r in th.as_tensor(table).detach().to("cpu").double().reshape(n, 8).tolist()]
    elif y0.dtype == th.float64:  # the order tests: no fp32 rounding of the weights, the grid's own float64 values
        rows = _weights([float(v) for v in grid.detach().cpu().double().tolist()], method)
    else:
        rows = [(r[:4], r[4:]) for r in multistep_table(grid, method).double().tolist()]
    tt = grid.to(y0.device)
    out = th.empty((n + 1,) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
    out[0] = y0
    y = p = y0
    k = []  # newest first
    for i in range(n):
        k.insert(0, func(tt[i].to(y0.dtype) if t_round else tt[i], p))
        del k[4:]
        a, b = rows[i]
        y = weight_sum(y, k, a) if used(a) else p
        out[i] = y
        p = weight_sum(y, k, b)
    out[n] = p
    return out
