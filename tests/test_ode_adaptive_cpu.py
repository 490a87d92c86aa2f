"""CPU: the step-size controller of lt_sample_ode_adaptive (csrc/samplers.hip), restated in plain scalars, against the host loop
``transport.integrators.adaptive_odeint`` on CPU fp32 tensors.

The C++ controller holds in fp32 what the host loop holds in 0-dim fp32 tensors (tcur + dt, tcur + fp32(alpha) dt, dt fp32(factor), the
interpolation argument x) and in double what the host loop computes in Python floats (the factor 0.9 / ratio ** (1 / order) with its
clamps, ratio == 0 -> 10).  ``replay`` below is that controller statement for statement with numpy fp32 scalars and Python floats; it is
fed the error ratios the host loop saw and must reproduce, word for word, the dt of every attempted step, every stage time (which pins
the accept / reject pattern: a rejected step is retried from the same tcur) and the x of every interpolation.  A controller that took
one of these expressions in the other precision fails here: ``test_the_precision_of_each_expression_matters`` shows it for each."""
import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport.integrators import _TABLEAUS, ADAPTIVE_METHODS, adaptive_odeint

f32 = np.float32


def initial_step(d0, d1, d2raw_of_h0, order):
    """_select_initial_step in scalars: d0, d1 fp32 norms, d2raw_of_h0(h0) the third norm (it needs h0 for its evaluation)"""
    d0, d1 = f32(d0), f32(d1)
    h0 = (f32(0.01) * d0) / d1 if (float(d0) >= 1e-5 and float(d1) >= 1e-5) else f32(1e-6)
    d2 = f32(d2raw_of_h0(h0)) / h0
    if float(d1) <= 1e-15 and float(d2) <= 1e-15:
        h1 = max(f32(1e-6), h0 * f32(1e-3))
    else:
        h1 = f32(float((f32(1.0) / max(d1, d2)) * f32(0.01)) ** (1.0 / order))
    return h0, min(f32(100.0) * h0, h1)


def replay(method, tgrid, dt, ratios, *, factor_in_fp32=False, dt_in_double=False, alpha_in_double=False):
    """the controller of lt_sample_ode_adaptive; the three switches move ONE expression each into the other precision"""
    alpha, _, _, _, _, order = _TABLEAUS[method]
    ratios = iter(ratios)
    tgrid = [f32(v) for v in tgrid]
    tcur = tprev = tgrid[0]
    dt = f32(dt)
    out = dict(dt=[], times=[], x=[], accepted=0, rejected=0)
    for next_t in tgrid[1:]:
        while next_t > tcur:
            t1 = tcur + dt
            assert t1 > tcur, "step size underflow"
            out["dt"].append(float(dt))
            for al in alpha:
                if alpha_in_double:
                    ti = t1 if al == 1.0 else f32(float(tcur) + al * float(dt))
                else:
                    ti = t1 if al == 1.0 else tcur + f32(al) * dt
                out["times"].append(float(ti))
            ratio = float(f32(next(ratios)))
            assert np.isfinite(ratio)
            if ratio <= 1.0:
                tprev, tcur = tcur, t1
                out["accepted"] += 1
            else:
                out["rejected"] += 1
            factor = 10.0
            if ratio != 0.0:
                dfactor = 1.0 if ratio < 1.0 else 0.2
                if factor_in_fp32:
                    factor = float(min(f32(10.0), max(f32(0.9) / f32(ratio) ** f32(1.0 / order), f32(dfactor))))
                else:
                    factor = min(10.0, max(0.9 / ratio ** (1.0 / order), dfactor))
            dt = f32(float(dt) * factor) if dt_in_double else dt * f32(factor)
        out["x"].append(float((next_t - tprev) / (tcur - tprev)))
    assert next(ratios, None) is None, "the host loop attempted more steps"
    return out


def host_loop(method, rhs, y0, tgrid, rtol, atol, first_step):
    """adaptive_odeint with everything the controller sees or decides recorded"""
    times, norms, st = [], [], {}

    def func(t, y):
        times.append(float(t))
        return rhs(y)

    def norm(x):
        v = x.float().pow(2).mean().sqrt()
        norms.append(float(v))
        return v

    out = adaptive_odeint(func, y0, tgrid, method=method, rtol=rtol, atol=atol, stats=st, norm=norm, first_step=first_step)
    return out, times, norms, st


ROT = torch.tensor([[0.0, 1.0], [-1.0, 0.0]])
RHS = {"decay": lambda y: -2.0 * y, "rotation": lambda y: y @ ROT.T}
GRID = torch.tensor([0.0, 0.3, 0.35, 1.0, 2.5])  # fp32; two points inside one step, unequal intervals


@pytest.mark.parametrize("method", ADAPTIVE_METHODS)
@pytest.mark.parametrize("problem", ["decay", "rotation"])
def test_controller_restatement_reproduces_the_host_loop_word_for_word(method, problem):
    y0 = torch.tensor([[1.5, -0.75]], dtype=torch.float32)
    first_step = 3.0  # far beyond what rtol 1e-3 allows at |lambda| = 1..2: the first attempt must be rejected
    out, times, norms, st = host_loop(method, RHS[problem], y0, GRID, 1e-3, 1e-6, first_step)
    assert len(norms) == st["accepted"] + st["rejected"] == len(st["dt"])  # a given first step: no heuristic norms, one ratio per attempt
    assert st["rejected"] >= 1 and norms[0] > 1.0, "the case was built to contain a rejected step"
    assert st["nfe"] == 1 + len(_TABLEAUS[method][0]) * len(st["dt"]) and st["first_step"] == first_step
    got = replay(method, GRID.tolist(), first_step, norms)
    assert got["dt"] == st["dt"]
    assert got["times"] == times[1:]
    assert (got["accepted"], got["rejected"]) == (st["accepted"], st["rejected"])
    # x of every interpolation: the host loop's (next_t - tprev) / (tcur - tprev) on 0-dim fp32 tensors, with tprev / tcur read off its own
    # stage times (every tableau's last stage sits at t1; an accepted t1 is the base of the next attempt)
    S = len(_TABLEAUS[method][0])
    t1 = [times[1 + i * S + S - 1] for i in range(len(st["dt"]))]
    acc = [r <= 1.0 for r in norms]
    tprev = tcur = float(GRID[0])
    k, xs = 0, []
    for nt in GRID[1:]:
        while float(nt) > tcur:
            if acc[k]:
                tprev, tcur = tcur, t1[k]
            k += 1
        xs.append(float((nt - torch.tensor(tprev)) / (torch.tensor(tcur) - torch.tensor(tprev))))
    assert k == len(t1) and got["x"] == xs
    assert any(x < 1.0 for x in xs), "no grid point fell inside a step: the dense output was not exercised"


@pytest.mark.parametrize("method", ADAPTIVE_METHODS)
def test_ratio_zero_branch_and_the_initial_step_heuristic(method):
    """y' = -2 y from y0 = 0: every slope is zero, the error ratio is exactly 0 and every step multiplies dt by 10; the heuristic takes
    its small-slope branch (h0 = 1e-6, h1 = max(1e-6, h0 1e-3)) - the one branch of it without a device pow"""
    y0 = torch.zeros(1, 3, dtype=torch.float32)
    grid = torch.tensor([0.0, 0.5, 1.0])
    out, times, norms, st = host_loop(method, RHS["decay"], y0, grid, 1e-3, 1e-6, None)
    order = _TABLEAUS[method][5]
    h0, dt0 = initial_step(norms[0], norms[1], lambda h0: norms[2], order)
    assert float(h0) == float(f32(1e-6)) and float(dt0) == st["first_step"] == float(f32(1e-6))
    assert times[1] == float(f32(0.0) + h0)
    ratios = norms[3:]
    assert ratios and all(r == 0.0 for r in ratios), "the case was built to take the ratio == 0 branch"
    got = replay(method, grid.tolist(), dt0, ratios)
    assert got["dt"] == st["dt"] and got["times"] == times[2:]
    assert got["rejected"] == st["rejected"] == 0 and got["accepted"] == st["accepted"] >= 6
    d = [f32(v) for v in st["dt"]]
    assert all(d[i + 1] == d[i] * f32(10.0) for i in range(len(d) - 1))
    assert torch.equal(out, torch.zeros_like(out))


def test_the_precision_of_each_expression_matters():
    """each expression of the controller, moved into the other precision, no longer reproduces the host loop: the finding of which is
    which is pinned by a case that tells them apart (dopri5 on the rotation, a tight tolerance: many steps, irregular ratios)"""
    y0 = torch.tensor([[1.5, -0.75]], dtype=torch.float32)
    grid = torch.linspace(0.0, 6.0, 9)
    _, times, norms, st = host_loop("dopri5", RHS["rotation"], y0, grid, 1e-5, 1e-7, 2.0)
    assert st["rejected"] >= 1 and len(st["dt"]) >= 12
    ok = replay("dopri5", grid.tolist(), 2.0, norms)
    assert ok["dt"] == st["dt"] and ok["times"] == times[1:]
    for switch in ("factor_in_fp32", "dt_in_double", "alpha_in_double"):
        try:
            other = replay("dopri5", grid.tolist(), 2.0, norms, **{switch: True})
            same = other["dt"] == st["dt"] and other["times"] == times[1:]
        except (AssertionError, StopIteration):  # the step sequence left the recorded one altogether
            same = False
        assert not same, f"{switch}: this case does not tell the two precisions apart"


def test_first_step_and_stats_leave_the_default_behaviour_alone():
    y0 = torch.tensor([[1.5, -0.75]], dtype=torch.float32)
    a = adaptive_odeint(lambda t, y: -2.0 * y, y0, GRID, rtol=1e-4, atol=1e-6)
    st = {}
    b = adaptive_odeint(lambda t, y: -2.0 * y, y0, GRID, rtol=1e-4, atol=1e-6, stats=st)
    assert torch.equal(a, b) and st["nfe"] == 2 + 6 * len(st["dt"]) and st["dt"][0] == st["first_step"]
    c = adaptive_odeint(lambda t, y: -2.0 * y, y0, GRID, rtol=1e-4, atol=1e-6, first_step=st["first_step"])
    assert torch.equal(a, c)


def test_new_symbols_are_in_the_binding_table_and_the_headers():
    new = ["lt_sample_ode_adaptive", "lt_op_rk_stage", "lt_op_rk_error_norm", "lt_op_rk_dense", "lt_op_rk_interp", "lt_op_rms_norm"]
    declared = _lib.declared_symbols()
    for name in new:
        assert name in _lib._SIGNATURES, name
        assert name in declared, name
    text = _lib.header_text()
    for name, value in (("LT_ODE_DOPRI5", 3), ("LT_ODE_BOSH3", 4), ("LT_ODE_FEHLBERG2", 5), ("LT_ODE_ADAPTIVE_HEUN", 6)):
        assert f"#define {name} {value}" in text and getattr(_lib, name) == value
    assert _lib.LT_ODE_DOPRI5 == _lib.LT_ODE_RK4 + 1
    assert sorted(_lib.ODE_ADAPTIVE_METHODS) == sorted(ADAPTIVE_METHODS)
    assert f"#define LT_RK_WS_BYTES {_lib.LT_RK_WS_BYTES}" in text and f"#define LT_RK_MAX_SLOPES {_lib.LT_RK_MAX_SLOPES}" in text
    assert _lib.LT_RK_MAX_SLOPES == max(len(tb[2]) for tb in _TABLEAUS.values())
