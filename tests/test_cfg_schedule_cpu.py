"""CPU: guidance schedules - lt_sample_ode_cfg_schedule, transport/guidance.py.  No GPU.

* ``stage_times`` equals, as fp32 words, the times a recording function sees inside ``fixed_grid_odeint``;
* ``cfg_table`` for an interval holds the scale exactly where ``lo <= t_stage < hi`` (both edges hit by a stage time) and 1.0 elsewhere;
* the host loop around a torch toy model: a constant table is ``fixed_grid_odeint`` around ``forward_with_cfg``, and ``forward`` runs on the
  B' cond rows exactly at the ``w == 1`` stages;
* the headers declare the entries, the library exports them and the ctypes binding has their arity; argument errors come back by name."""
import ctypes as C
import re

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.integrators import fixed_grid_odeint
from lumina_t2x_amd.transport.mini import ODE

NEW = ("lt_sample_ode_cfg_schedule", "lt_last_eval_rows", "lt_op_unpatchify_cfg_dev")
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _grids():
    return {"shifted": ODE(7, "euler", 4.0).t, "cut": ODE(9, "euler", 4.0, strength=0.6).t, "plain": ODE(5, "euler").t}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_stage_times_are_the_times_fixed_grid_odeint_hands_its_function(method, dtype):
    for name, tgrid in _grids().items():
        assert tgrid.dtype == torch.float32 and len(tgrid) >= 2 and (name != "cut" or float(tgrid[0]) > 0)
        seen = []

        def func(t, y):
            assert t.dtype == dtype  # torchdiffeq casts the time to the state dtype
            seen.append(float(t.to(torch.float32)))
            return -y

        fixed_grid_odeint(func, torch.ones(2, 3, dtype=dtype), tgrid, method=method)
        want = torch.tensor(seen, dtype=torch.float32)
        got = G.stage_times(tgrid, method, dtype)
        assert got.dtype == torch.float32 and got.numel() == (len(tgrid) - 1) * STAGES[method]
        assert torch.equal(_bits(got), _bits(want)), (name, method, dtype)
        if dtype == torch.bfloat16:  # without the rounding they are the fp32 state's times
            assert torch.equal(_bits(G.stage_times(tgrid, method, dtype, t_round=False)), _bits(G.stage_times(tgrid, method, torch.float32)))


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_cfg_table_of_an_interval_is_half_open_on_the_unrounded_stage_times(method):
    tgrid = ODE(7, "euler", 4.0).t
    ts = G.stage_times(tgrid, method, torch.float32, False)
    # lo and hi ARE stage times: the stage at lo is guided, the stage at hi is not
    lo, hi = float(ts[STAGES[method]]), float(ts[-2])
    assert lo < hi
    table = G.cfg_table(tgrid, method, 4.0, interval=(lo, hi))
    assert table.dtype == torch.float32 and table.shape == ts.shape
    inside = (ts >= lo) & (ts < hi)
    assert bool(inside.any()) and bool((~inside).any())
    assert torch.equal(table, torch.where(inside, torch.tensor(4.0), torch.tensor(1.0)))
    assert float(table[STAGES[method]]) == 4.0 and float(table[-2]) == 1.0 and float(table[0]) == 1.0
    # the table does not depend on the state dtype: bf16 rounding would move a stage across the edge
    assert torch.equal(table, G.cfg_table(tgrid.clone(), method, 4.0, interval=(lo, hi)))
    # no interval: the scale everywhere; a callable: its values at the stage times
    assert torch.equal(G.cfg_table(tgrid, method, 2.5), torch.full_like(ts, 2.5))
    ramp = G.cfg_table(tgrid, method, 4.0, schedule=lambda t: 1.0 + 3.0 * (1.0 - t))
    assert torch.equal(ramp, torch.tensor([1.0 + 3.0 * (1.0 - t) for t in ts.tolist()], dtype=torch.float32))
    lin = G.cfg_table(tgrid, method, 4.0, schedule=G.linear_schedule(4.0, float(tgrid[0]), float(tgrid[-1])))
    cos = G.cfg_table(tgrid, method, 4.0, schedule=G.cosine_schedule(4.0, float(tgrid[0]), float(tgrid[-1])))
    for tab in (lin, cos):
        assert float(tab[0]) == 4.0 and bool((tab[1:] <= tab[:-1]).all()) and bool((tab >= 1.0).all())
    with pytest.raises(ValueError, match="not finite"):
        G.cfg_table(tgrid, method, float("nan"))
    with pytest.raises(ValueError, match="fixed-grid"):
        G.cfg_table(tgrid, "dopri5", 4.0)


class Toy:
    """a torch 'model': the guidance expression of the reference on a function of (x, t, y), and a log of every call"""

    def __init__(self):
        self.calls = []

    def net(self, x, t, y):
        return torch.tanh(x * y.view(-1, 1, 1, 1).to(x.dtype)) - t.view(-1, 1, 1, 1).to(x.dtype) * x

    def forward(self, x, t, y):
        self.calls.append(("forward", x.shape[0], float(t[0]), tuple(y.tolist())))
        assert t.dtype == torch.float32 and t.shape[0] == x.shape[0] == y.shape[0]
        return self.net(x, t, y)

    def forward_with_cfg(self, x, t, y, cfg_scale, gain=1.0):
        self.calls.append(("cfg", x.shape[0], float(t[0]), float(cfg_scale)))
        half = x[: len(x) // 2]
        out = self.net(torch.cat([half, half]), t, y) * gain
        cond, unc = out.chunk(2)
        g = unc + cfg_scale * (cond - unc)
        return torch.cat([g, g])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_host_loop_is_fixed_grid_odeint_and_calls_forward_on_the_cond_rows_at_scale_one(method, dtype):
    tgrid = ODE(6, method, 4.0).t
    n = (len(tgrid) - 1) * STAGES[method]
    g = torch.Generator().manual_seed(2)
    z = torch.randn(2, 3, 4, 4, generator=g).to(dtype).repeat(2, 1, 1, 1)
    y = torch.tensor([0.5, -1.25, 2.0, 0.75])
    toy = Toy()
    # a constant table: fixed_grid_odeint around forward_with_cfg
    got = G.sample_cfg_schedule(toy, z, tgrid, torch.full((n,), 3.0), method, y=y, gain=1.0)
    assert [c[0] for c in toy.calls] == ["cfg"] * n

    def fn(t, yy):
        return toy.forward_with_cfg(yy, torch.ones(yy.size(0)) * t, y, 3.0)

    want = fixed_grid_odeint(fn, z, tgrid, method=method)
    assert got.shape == want.shape and got.dtype == dtype and torch.equal(_bits(got.float()), _bits(want.float()))
    # a table with both kinds of stage: forward on the B' cond rows and their labels exactly where w == 1, at the stage's time
    table = torch.tensor([1.0 if i % 3 == 1 else 1.0 + i for i in range(n)])
    toy.calls.clear()
    mixed = G.sample_cfg_schedule(toy, z, tgrid, table, method, y=y, gain=1.0)
    times = G.stage_times(tgrid, method, dtype).tolist()
    assert len(toy.calls) == n
    for i, c in enumerate(toy.calls):
        if float(table[i]) == 1.0:
            assert c == ("forward", 2, times[i], (0.5, -1.25)), (i, c)
        else:
            assert c == ("cfg", 4, times[i], float(table[i])), (i, c)
    assert bool(torch.isfinite(mixed.float()).all()) and not torch.equal(mixed[-1], got[-1])
    # through the transport front end (a CPU state runs the host loop)
    o = ODE(6, method, 4.0)
    assert torch.equal(o.sample(z, toy.forward_with_cfg, cfg_table=table, y=y, gain=1.0), mixed)
    with pytest.raises(ValueError, match="entries"):
        G.sample_cfg_schedule(toy, z, tgrid, table[:-1], method, y=y)
    with pytest.raises(ValueError, match="even batch"):
        G.sample_cfg_schedule(toy, z[:3], tgrid, table, method, y=y[:3])
    with pytest.raises(ValueError, match="not finite"):
        G.sample_cfg_schedule(toy, z, tgrid, torch.full((n,), float("inf")), method, y=y)


def test_headers_declare_the_calls_and_the_binding_matches():
    lib = _lib.load()
    text = _lib.header_text()
    for name in NEW:
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        params = [p.strip() for p in decl.group(2).split(",")]
        res, args = _lib._SIGNATURES[name]
        assert res is (C.c_int64 if decl.group(1) == "int64_t" else C.c_int32) and len(args) == len(params), (name, len(args), params)
        for p, a in zip(params, args):
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            elif p.startswith("float"):
                assert a is C.c_float, (name, p, a)
            else:
                assert p.startswith("int32_t") and a is C.c_int32, (name, p, a)
    assert re.search(r"lt_sample_ode_cfg_schedule\(lt_engine\* e, const void\* z_dev, void\* traj_dev, void\* final_dev, const float\* tgrid_host, "
                     r"int32_t n_grid,\s+int32_t method, const float\* cfg_host, int32_t t_round_to_state_dtype, const lt_step_args\* a, void\* stream\)",
                     text)


def test_argument_errors_come_back_by_name_without_a_device():
    lib = _lib.load()
    a = _lib.LtStepArgs(batch=2, io_dtype=_lib.LT_BF16)
    grid = (C.c_float * 2)(0.0, 1.0)
    tab = (C.c_float * 4)(4.0, 4.0, 4.0, 4.0)
    one = C.c_void_p(64)  # never dereferenced: every call below is refused before it reads anything
    assert lib.lt_sample_ode_cfg_schedule(one, one, None, one, grid, 2, 0, None, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_cfg_schedule: null argument" in lib.lt_last_error()
    assert lib.lt_sample_ode_cfg_schedule(None, one, None, one, grid, 2, 0, tab, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_cfg_schedule: null argument" in lib.lt_last_error()
    assert lib.lt_last_eval_rows(None) == -1
