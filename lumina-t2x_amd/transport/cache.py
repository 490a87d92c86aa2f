"""Step caching by the TeaCache rule: a fixed-grid trajectory whose evaluations may leave the block stack out.

The reference has no such sampler; this module is the definition ``lt_sample_ode_cached`` is held to.  An evaluation of an engine-backed model
splits into a *head* (patchify, embedding, conditioning, the first pre-norm + modulate: the bf16 tensor ``h`` that enters block 0), the *stack*
of L blocks, and a *tail* (final norm + modulate, final projection, guidance).  TeaCache compares ``h`` between evaluations:

    S1 = sum |h_j - h_{j-1}|        S0 = sum |h_{j-1}|        rel = S1 / S0        acc += poly(rel)

(float64 throughout) and runs the stack only when ``acc`` has reached the threshold; otherwise the token stream after the stack is taken to be
``x0_j + r`` with ``r = x_L - x_0`` of the last evaluation that ran it.  The first and the last evaluation always run.

``poly`` has five coefficients, highest power first; the default ``(0, 0, 0, 1, 0)`` is the identity.  Published coefficient sets exist for this
model family, but none has been verified here against a trained checkpoint, so none is built in.  No image-quality claim is made.

The host loop needs the head of an evaluation on its own (the probe), which only the engine offers: a model that is not engine-backed is
refused by name.
"""
from __future__ import annotations

import math

import torch as th

from .integrators import ADAPTIVE_METHODS, FIXED_GRID_METHODS, _call
from .multistep import MULTISTEP_METHODS

IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0)
_STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


def check_cache_args(threshold, coefficients=IDENTITY):
    """``(threshold as the fp32 value the engine takes, five float64 coefficients)``; ValueError by name otherwise"""
    try:
        thr = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"teacache threshold {threshold!r} is not a number") from None
    if not thr >= 0.0:
        raise ValueError(f"teacache threshold {thr} is not a number >= 0")
    thr = float(th.tensor(thr, dtype=th.float32))  # (the C ABI takes a float)
    try:
        coef = tuple(float(c) for c in coefficients)
    except TypeError:
        raise ValueError("teacache coefficients: five numbers, highest power first") from None
    if len(coef) != 5:
        raise ValueError(f"teacache coefficients: five numbers, highest power first, got {len(coef)}")
    if not all(math.isfinite(c) for c in coef):
        raise ValueError(f"teacache coefficients must be finite, got {coef}")
    return thr, coef


def check_cache_method(method):
    """the stages of a method step caching serves; the multistep and adaptive solvers are refused by name"""
    if method in MULTISTEP_METHODS:
        raise ValueError(f"step caching (teacache) is not built for the multistep method '{method}' (served: {', '.join(FIXED_GRID_METHODS)})")
    if method in ADAPTIVE_METHODS:
        raise ValueError(f"step caching (teacache) is not built for the adaptive solver '{method}' (served: {', '.join(FIXED_GRID_METHODS)})")
    if method not in FIXED_GRID_METHODS:
        raise ValueError(f"step caching (teacache) is built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not '{method}'")
    return _STAGES[method]


# what step caching is refused together with, by name (combining them is later work): option -> the words the refusal carries
REFUSED_WITH = {
    "cfg_interval": "a guidance interval (cfg_interval)",
    "cfg_schedule": "a guidance schedule (cfg_schedule)",
    "cfg_table": "a guidance table (cfg_table)",
    "cfg_rescale": "rescaled guidance (cfg_rescale)",
    "cfg_norm_limit": "norm-limited guidance (cfg_norm_limit)",
    "cfg_reuse": "guidance reuse (cfg_reuse)",
    "slg": "skip-layer guidance (slg)",
    "mask": "an inpainting mask",
    "packed": "a packed batch (a list of latents)",
}


def refuse_with_teacache(method="euler", **options):
    """ValueError naming the first option in ``options`` that is switched on (``None`` / ``False`` / ``0`` / ``inf`` for ``cfg_norm_limit`` /
    an empty sequence: off) and that step caching does not serve; then the method's refusals"""
    for name, value in options.items():
        if name not in REFUSED_WITH:
            raise TypeError(f"refuse_with_teacache: unknown option '{name}'")
        off = value is None or value is False or (isinstance(value, (int, float)) and (value == 0 or (name == "cfg_norm_limit" and value == math.inf)))
        if not off and hasattr(value, "__len__") and len(value) == 0:
            off = True
        if not off:
            raise ValueError(f"step caching (teacache) is not served together with {REFUSED_WITH[name]}")
    check_cache_method(method)


def poly(rel, coef):
    """Horner in Python floats (float64, every operation rounds)"""
    p = coef[0]
    for c in coef[1:]:
        p = p * rel + c
    return p


class CacheController:
    """The accumulator of one trajectory of ``ncalls`` evaluations.  ``step(j, S1, S0) -> (rel, acc after the add, ran)``: the stack runs on the
    first and on the last evaluation (rel reported 0, the sums are not looked at), when ``S0 == 0`` (rel reported inf, ``acc`` takes nothing),
    and when ``not (acc < threshold)``; whenever it runs ``acc`` returns to 0."""

    def __init__(self, ncalls, threshold, coefficients=IDENTITY):
        self.thr, self.coef = check_cache_args(threshold, coefficients)
        self.ncalls = int(ncalls)
        self.acc = 0.0

    def reads(self, j):
        """whether evaluation ``j`` looks at the indicator at all"""
        return 0 < j < self.ncalls - 1

    def step(self, j, S1=0.0, S0=0.0):
        rel, run = 0.0, True
        if self.reads(j):
            if S0 == 0.0:
                rel = math.inf
            else:
                rel = S1 / S0
                self.acc += poly(rel, self.coef)
                run = not (self.acc < self.thr)
        seen = self.acc
        if run:
            self.acc = 0.0
        return rel, seen, run


def indicator_sums(h, h_prev):
    """``(S1, S0)`` of two bf16 tensors in float64 (torch's reduction order; the kernel's differs by at most ``sum_bound`` relative)"""
    a, b = h.double().reshape(-1), h_prev.double().reshape(-1)
    return float((a - b).abs().sum()), float(b.abs().sum())


def sum_bound(n):
    """relative distance two float64 summations of the same ``n`` non-negative terms can have: each is within ``(n - 1) u`` of the exact sum,
    ``u = 2^-53`` (every partial sum is non-negative, so no cancellation); the quotient of two such sums: twice that, to first order"""
    return 2.0 * n * 2.0 ** -53


class EngineEvaluator:
    """the three parts of an evaluation on a prepared engine: ``probe(x, t) -> (S1, S0)``, then ``run(x, t)`` or ``reuse(x, t)`` of the same
    ``x`` and ``t`` (``DiTEngine.forward_cached``)"""

    def __init__(self, engine, use_cfg, args):
        self.engine, self.use_cfg, self.args = engine, bool(use_cfg), dict(args)

    def probe(self, x, t):
        return self.engine.forward_cached(x, t, "probe", use_cfg=self.use_cfg, **self.args)

    def run(self, x, t):
        return self.engine.forward_cached(x, t, "run", use_cfg=self.use_cfg, **self.args)

    def reuse(self, x, t):
        return self.engine.forward_cached(x, t, "reuse", use_cfg=self.use_cfg, **self.args)


def sample_teacache(ev, z, tgrid, method="euler", *, threshold=0.0, coefficients=IDENTITY, t_round=True, stats=None):
    """The trajectory under step caching on the host: every state ``[len(tgrid), *z.shape]``.  This IS the definition ``lt_sample_ode_cached``
    is held to, state for state.  ``ev``: an evaluator with ``probe`` / ``run`` / ``reuse`` (``EngineEvaluator``); per evaluation the loop probes,
    asks the controller, and runs the stack or reuses the residual.  The loop around the evaluations is ``fixed_grid_odeint``'s, statement for
    statement.  ``stats`` (a list): receives ``(rel, acc after the add, ran)`` of every evaluation."""
    if isinstance(z, (list, tuple)):
        raise ValueError("step caching (teacache) takes a tensor state; a packed batch (a list of latents) is not served")
    if not all(hasattr(ev, k) for k in ("probe", "run", "reuse")):
        raise TypeError("step caching (teacache) needs an engine-backed model: the host loop probes the head of every evaluation, which only "
                        "the engine offers")
    stages = check_cache_method(method)
    t = tgrid if isinstance(tgrid, th.Tensor) else th.tensor(list(tgrid), dtype=th.float32)
    t = t.detach().to(z.device, th.float32)
    if t.dim() != 1 or len(t) < 2:
        raise ValueError("step caching (teacache) needs a 1-D grid of at least 2 points")
    ctl = CacheController((len(t) - 1) * stages, threshold, coefficients)
    call = [0]

    def func(tt, y):
        tvec = th.ones(y.size(0)).to(y.device) * tt  # fp32 [B] (integrators.py: ode.sample)
        j = call[0]
        call[0] += 1
        S1, S0 = ev.probe(y, tvec)
        rel, seen, run = ctl.step(j, S1, S0)
        if stats is not None:
            stats.append((rel, seen, run))
        return ev.run(y, tvec) if run else ev.reuse(y, tvec)

    def f(tt, y):
        return _call(func, tt, y) if t_round else func(tt, y)

    # fixed_grid_odeint's loop (integrators.py), statement for statement
    out = th.empty((len(t),) + tuple(z.shape), dtype=z.dtype, device=z.device)
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
