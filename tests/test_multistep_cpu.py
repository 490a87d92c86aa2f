"""CPU: linear multistep ODE sampling - ab2 / ab3 / abm2 / abm3, transport/multistep.py, lt_sample_ode_multistep.  No GPU.

* weights: every row sums to its interval, the uniform grid gives the textbook Adams weights, ab3 integrates t^2 exactly from step 2 on;
* order and usefulness in float64 on a non-linear problem over the time-shifted grid: observed orders above their floors, abm2 / abm3 below
  midpoint's error at equal evaluations;
* routing: a plain callable runs the host loop with exactly N evaluations, masks are refused by name, torchdiffeq's Adams names still raise;
* the torch expressions of a step equal the float64 restatement of the rounding chain (tests/exact_multistep.py) word for word;
* the headers declare the calls, the binding has their arity, and the host-side argument errors come back by name without a device."""
import ctypes as C
import math
import re

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport import integrators as I
from lumina_t2x_amd.transport import masked as MK
from lumina_t2x_amd.transport import multistep as MS
from lumina_t2x_amd.transport.mini import ODE

import exact_multistep as X

NEW = ("lt_sample_ode_multistep", "lt_sample_ode_multistep_packed", "lt_op_ode_multistep")
METHODS = MS.MULTISTEP_METHODS


def _shifted(N, s=3.0, dtype=torch.float32):
    u = torch.linspace(0, 1, N + 1, dtype=dtype)
    return u / (u + s - s * u)


# ---- weights -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_every_row_sums_to_its_interval(method):
    assert MS.MULTISTEP_METHODS == ("ab2", "ab3", "abm2", "abm3")
    t = _shifted(9)
    g = [float(v) for v in t.tolist()]
    tab = MS.multistep_table(t, method)
    assert tab.shape == (9, 8) and tab.dtype == torch.float32
    rows64 = MS.multistep_weights(t, method)
    for i in range(9):
        a64, b64 = rows64[i]
        # the float64 weights sum to the interval to float64 rounding; the fp32 row is their rounding, one half ulp per entry
        assert abs(sum(b64) - (g[i + 1] - g[i])) < 1e-14
        slack = sum(abs(float(torch.tensor(v, dtype=torch.float32)) - v) for v in b64) + 1e-14
        assert abs(float(tab[i, 4:].double().sum()) - (g[i + 1] - g[i])) <= slack
        assert all(float(torch.tensor(v, dtype=torch.float64).to(torch.float32)) == float(tab[i, 4 + j]) for j, v in enumerate(b64))
        if MS.is_corrector(method) and i >= 1:
            assert abs(sum(a64) - (g[i] - g[i - 1])) < 1e-14
            slack = sum(abs(float(torch.tensor(v, dtype=torch.float32)) - v) for v in a64) + 1e-14
            assert abs(float(tab[i, :4].double().sum()) - (g[i] - g[i - 1])) <= slack
        else:
            assert bool((tab[i, :4] == 0).all())
        q = 2 if method.endswith("2") else 3
        assert MS.used(tab[i, 4:].tolist()) == min(q, i + 1)
        assert MS.used(tab[i, :4].tolist()) == (min(q, i) + 1 if MS.is_corrector(method) and i >= 1 else 0)


def test_uniform_grid_gives_the_textbook_weights():
    h = 0.125  # a power of two: the weights below are exact in float64 up to the integration's own rounding
    t = torch.arange(9, dtype=torch.float32) * h
    close = lambda got, want: all(abs(a - b) < 1e-15 for a, b in zip(got, want))  # noqa: E731
    for method in METHODS:
        rows = MS.multistep_weights(t, method)
        assert close(rows[0][1], [h, 0, 0, 0]), method  # step 0 is Euler
        assert close(rows[0][0], [0, 0, 0, 0]), method
    ab2, ab3, abm2, abm3 = (MS.multistep_weights(t, m) for m in METHODS)
    for i in range(1, 8):
        assert close(ab2[i][1], [h * 1.5, -h * 0.5, 0, 0]), i
        assert close(abm2[i][1], ab2[i][1]) and close(abm3[i][1], ab3[i][1]), i
    assert close(ab3[1][1], [h * 1.5, -h * 0.5, 0, 0])
    for i in range(2, 8):
        assert close(ab3[i][1], [h * 23 / 12, -h * 16 / 12, h * 5 / 12, 0]), i
        assert close(abm2[i][0], [h * 5 / 12, h * 8 / 12, -h / 12, 0]), i
    for m in (abm2, abm3):  # the corrector of step 1 is the trapezoid rule
        assert close(m[1][0], [h / 2, h / 2, 0, 0])
    assert close(abm3[2][0], [h * 5 / 12, h * 8 / 12, -h / 12, 0])
    for i in range(3, 8):  # Adams-Moulton on four nodes
        assert close(abm3[i][0], [h * 9 / 24, h * 19 / 24, -h * 5 / 24, h / 24]), i
    want = torch.tensor([h * 9 / 24, h * 19 / 24, -h * 5 / 24, h / 24, h * 23 / 12, -h * 16 / 12, h * 5 / 12, 0.0], dtype=torch.float64)
    assert torch.allclose(MS.multistep_table(t, "abm3")[5].double(), want, rtol=2.0 ** -24, atol=0)  # one rounding to fp32


def test_ab3_integrates_a_quadratic_exactly_from_step_2_on():
    t = _shifted(8, dtype=torch.float64)
    calls = []

    def f(tt, y):
        calls.append(float(tt))
        return (tt * tt).reshape(1)

    out = MS.multistep_odeint(f, torch.zeros(1, dtype=torch.float64), t, "ab3")
    assert len(calls) == 8 and calls == [float(v) for v in t[:-1]]
    # steps 0 and 1 (Euler, two slopes) are not exact; from step 2 on every increment is the integral of t^2 over its interval
    for i in range(2, 8):
        inc = float(out[i + 1] - out[i])
        want = (float(t[i + 1]) ** 3 - float(t[i]) ** 3) / 3
        assert abs(inc - want) < 1e-15, (i, inc, want)
    assert abs(float(out[1] - out[0]) - float(t[1]) ** 3 / 3) > 1e-6


# ---- order and usefulness ------------------------------------------------------------------------------------------------------------
def _f(t, y):
    return torch.stack([-2 * t * y[0] + torch.cos(3 * t) * y[1], torch.sin(2 * t) - y[0] * y[1]])


_Y0 = torch.tensor([1.0, 0.5], dtype=torch.float64)
_REF = {}


def _reference():
    if "y" not in _REF:  # RK4, 20 000 steps, computed once
        y, n = _Y0.clone(), 20000
        h = 1.0 / n
        for i in range(n):
            t = torch.tensor(i * h, dtype=torch.float64)
            k1 = _f(t, y)
            k2 = _f(t + h / 2, y + h / 2 * k1)
            k3 = _f(t + h / 2, y + h / 2 * k2)
            k4 = _f(t + h, y + h * k3)
            y = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        _REF["y"] = y
    return _REF["y"]


def _err(method, N):
    key = (method, N)
    if key not in _REF:
        t = _shifted(N, dtype=torch.float64)
        if method in METHODS:
            y = MS.multistep_odeint(_f, _Y0, t, method)[-1]
        else:
            y = I.fixed_grid_odeint(_f, _Y0, t, method=method)[-1]
        _REF[key] = float((y - _reference()).abs().max())
    return _REF[key]


@pytest.mark.parametrize("method,floor", [("ab2", 1.8), ("abm2", 2.6), ("ab3", 3.0), ("abm3", 3.5)])
def test_observed_order_meets_its_floor(method, floor):
    orders = [math.log2(_err(method, N) / _err(method, 2 * N)) for N in (32, 64)]
    print(f"{method}: errors {[_err(method, N) for N in (32, 64, 128)]}, observed orders {orders} (floor {floor})")
    assert min(orders) >= floor, (method, orders)


@pytest.mark.parametrize("method", ["abm2", "abm3"])
def test_error_is_below_midpoint_at_equal_evaluations(method):
    for N in (16, 32, 64, 128):
        ours, mid = _err(method, N), _err("midpoint", N // 2)
        print(f"NFE {N}: {method} {ours:.3e}  midpoint {mid:.3e}")
        assert ours < mid, (method, N, ours, mid)


# ---- routing, refusals, tables -------------------------------------------------------------------------------------------------------
def test_a_plain_callable_runs_the_host_loop_with_exactly_n_calls():
    calls = []

    def model(x, t, **kw):
        calls.append((tuple(t.shape), float(t[0])))
        return -x

    z = torch.randn(2, 4, 4, 4, generator=torch.Generator().manual_seed(1))
    o = ODE(7, "abm2", 3.0)
    out = o.sample(z, model)
    assert out.shape == (7,) + tuple(z.shape) and len(calls) == 6
    assert [c[1] for c in calls] == [float(v) for v in o.t[:-1]] and all(c[0] == (2,) for c in calls)
    assert torch.equal(out, MS.multistep_odeint(lambda t, y: -y, z, o.t, "abm2")) and torch.equal(out[0], z)
    # the Sampler front end: the same loop around the velocity drift
    calls.clear()
    fn = Sampler(create_transport()).sample_ode(sampling_method="ab3", num_steps=7, time_shifting_factor=3.0)
    out2 = fn(z, model)
    assert len(calls) == 6 and out2.shape == out.shape
    assert torch.equal(out2, MS.multistep_odeint(lambda t, y: -y, z, fn.__self__.t, "ab3"))
    for m in METHODS:
        assert m in I.BUILT_METHODS and m not in I.NOT_BUILT_METHODS and m not in I.ALL_METHODS  # ALL_METHODS: torchdiffeq's names


def test_masked_sampling_with_a_multistep_method_is_refused_by_name():
    z = torch.zeros(2, 4, 4, 4)
    m = torch.ones(4, 4)
    for method in METHODS:
        with pytest.raises(NotImplementedError, match="multistep method .*discontinuous"):
            ODE(5, method).sample(z, lambda x, t: x, mask=m, x1=z, noise=z)
        with pytest.raises(NotImplementedError, match="multistep method .*discontinuous"):
            MK.sample_masked(lambda x, t: x, z, torch.linspace(0, 1, 5), z, z, z, method)
    with pytest.raises(ValueError, match="fixed-grid methods"):  # the refusal it was
        MK.sample_masked(lambda x, t: x, z, torch.linspace(0, 1, 5), z, z, z, "heun2")


def test_torchdiffeq_adams_names_still_raise_as_before():
    z = torch.zeros(1, 2)
    for name in ("explicit_adams", "implicit_adams", "fixed_adams"):
        assert name in I.NOT_BUILT_METHODS and name not in I.BUILT_METHODS
        with pytest.raises(NotImplementedError, match=f"ODE method '{name}' of torchdiffeq is not built here"):
            ODE(4, name).sample(z, lambda x, t: x)
        with pytest.raises(NotImplementedError, match="not built here"):
            Sampler(create_transport()).sample_ode(sampling_method=name, num_steps=4)(z, lambda x, t: x)
    with pytest.raises(ValueError, match="unknown multistep method"):
        MS.multistep_table(torch.linspace(0, 1, 4), "ab4")
    # the hints a user sees name the multistep methods too
    with pytest.raises(NotImplementedError, match="built: .*heun3.*ab2, ab3, abm2, abm3"):
        ODE(4, "dopri8").sample(z, lambda x, t: x)
    with pytest.raises(ValueError, match="unknown ODE method 'rk45' .*multistep methods: ab2, ab3, abm2, abm3"):
        ODE(4, "rk45").sample(z, lambda x, t: x)


@pytest.mark.parametrize("front", ["mini", "sampler"])
def test_host_routes_pass_t_round_on(front):
    """with a bf16 state the host loop hands the model the grid time rounded to bf16, or - t_round_to_state_dtype = False - as it is"""
    z = torch.zeros(2, 4, 2, 2, dtype=torch.bfloat16)
    seen = []

    def model(x, t, **kw):
        seen.append(float(t[0]))
        return x

    if front == "mini":
        solver = ODE(5, "ab2", 3.0)
        fn = solver.sample
    else:
        fn = Sampler(create_transport()).sample_ode(sampling_method="ab2", num_steps=5, time_shifting_factor=3.0)
        solver = fn.__self__
    grid = [float(v) for v in solver.t[:-1]]
    rounded = [float(v) for v in solver.t[:-1].to(torch.bfloat16)]
    assert grid != rounded
    fn(z, model)
    assert seen == rounded
    seen.clear()
    solver.t_round_to_state_dtype = False
    fn(z, model)
    assert seen == grid


def test_cfg_table_has_one_entry_per_evaluation():
    t = _shifted(6)
    for method in METHODS:
        tab = G.cfg_table(t, method, 4.0, interval=(0.1, 0.7))
        assert tab.shape == (6,) and tab.tolist() == G.cfg_table(t, "euler", 4.0, interval=(0.1, 0.7)).tolist()
        assert 0 < int((tab == 4.0).sum()) < 6
        assert G.check_table(tab, t, method).shape == (6,)
        with pytest.raises(ValueError, match="entries"):
            G.check_table(torch.ones(12), t, method)
    with pytest.raises(ValueError, match="fixed-grid methods"):  # the refusal it was
        G.cfg_table(t, "heun2", 4.0)


def test_host_loop_with_a_table_calls_forward_at_scale_one():
    class Toy:
        cfg_channels = 3

        def __init__(self):
            self.calls = []

        def forward(self, x, t, cap):
            self.calls.append(("f", x.shape[0]))
            return -x * cap.view(-1, 1, 1, 1)

        def forward_with_cfg(self, x, t, cap, cfg_scale):
            self.calls.append(("g", x.shape[0], cfg_scale))
            return -x * cfg_scale

    toy = Toy()
    z = torch.randn(2, 4, 2, 2, generator=torch.Generator().manual_seed(2))
    o = ODE(4, "ab2")
    out = o.sample(z, toy.forward_with_cfg, cfg_table=[2.0, 1.0, 3.0], cap=torch.ones(2), cfg_scale=9.0)
    assert out.shape == (4,) + tuple(z.shape)
    assert toy.calls == [("g", 2, 2.0), ("f", 1), ("g", 2, 3.0)]


# ---- chain ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_host_step_equals_the_float64_chain_word_for_word(dtype):
    n = 4096
    y_prev, *ks = X.operands(n, dtype, 5)
    tab = MS.multistep_table(_shifted(6), "abm3")
    cases = [(tab[i, :4].tolist(), tab[i, 4:].tolist(), int(i >= 1)) for i in range(6)]
    cases += [(list(X.MIDPOINT_WEIGHTS), list(X.MIDPOINT_WEIGHTS[::-1]), 1), ([0.0] * 4, [X.FMA_WEIGHT, 0.0, 0.0, 0.0], 0)]
    for a, b, has_corr in cases:
        y, p = X.host_step(y_prev, ks, a, b, has_corr)
        wy, wp = X.chain64(y_prev, ks, a, b, has_corr, dtype)
        assert y.dtype == p.dtype == dtype
        assert torch.equal(X.bits(y), X.bits(wy)) and torch.equal(X.bits(p), X.bits(wp)), (dtype, a, b)
    if dtype == torch.float32:  # the fma case separates the two arithmetics: the chain gives 0 where one fused rounding gives 2^-24
        _, p = X.host_step(y_prev, ks, [0.0] * 4, [X.FMA_WEIGHT, 0.0, 0.0, 0.0], 0)
        fused = X.fused64(y_prev, ks[0], X.FMA_WEIGHT)
        assert bool((p[1::4] == 0).all()) and bool((fused[1::4] == 2.0 ** -24).all())
    else:  # the midpoint lanes: dropping the product's own rounding moves words
        a = list(X.MIDPOINT_WEIGHTS)
        y, _ = X.host_step(y_prev, ks, a, a, 1)
        lazy = (y_prev.double() + sum(k.double() * c for k, c in zip(ks, a))).to(torch.bfloat16)
        assert int((X.bits(y)[0::4] != X.bits(lazy)[0::4]).sum()) > n // 64


def test_bf16_host_loop_equals_the_chain_restated_step_by_step():
    """a whole bf16 trajectory of the host loop against the float64 chain applied step by step to the same slopes"""
    t = _shifted(6)
    g = torch.Generator().manual_seed(9)
    z = torch.randn(512, generator=g).to(torch.bfloat16)
    W = torch.randn(512, generator=g).to(torch.bfloat16)
    slopes = []

    def f(tt, y):
        slopes.append((y * W + tt).to(torch.bfloat16))
        return slopes[-1]

    for method in METHODS:
        slopes.clear()
        out = MS.multistep_odeint(f, z, t, method)
        tab = MS.multistep_table(t, method)
        y = p = z
        for i in range(6):
            ks = slopes[i::-1][:4]
            a, b = tab[i, :4].tolist(), tab[i, 4:].tolist()
            has_corr = int(MS.used(a) > 0)  # without a corrector weight y_i is the predicted state the slope was taken at
            y, p = X.chain64(y if has_corr else p, ks, a, b, has_corr, torch.bfloat16)
            assert torch.equal(X.bits(out[i]), X.bits(y)), (method, i)
        assert torch.equal(X.bits(out[6]), X.bits(p)), method


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_headers_declare_the_calls_and_the_binding_matches():
    lib = _lib.load()
    text = _lib.header_text()
    for name in NEW:
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = _lib._SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), (name, len(args), params)
    assert (_lib.LT_ODE_AB2, _lib.LT_ODE_AB3, _lib.LT_ODE_ABM2, _lib.LT_ODE_ABM3) == (32, 33, 34, 35)
    for name, code in _lib.ODE_MULTISTEP_METHODS.items():
        assert re.search(rf"#define LT_ODE_{name.upper()} {code}\b", _lib.header_text(strip_comments=False)), name


def test_host_side_argument_errors_come_back_by_name_without_a_device():
    lib = _lib.load()
    a = _lib.LtStepArgs(batch=2, io_dtype=_lib.LT_BF16, latent_h=16, latent_w=16)
    grid = (C.c_float * 3)(0.0, 0.5, 1.0)
    F = C.c_float * 16
    good = F(*MS.multistep_table([0.0, 0.5, 1.0], "abm2").reshape(-1).tolist())
    nan = F(*good)
    nan[12] = float("nan")
    early = F(*good)
    early[5] = 0.25  # a second corrector slope at step 0... row 0 names 2 slopes with 1 evaluation made
    one = C.c_void_p(64)  # never dereferenced: every call below is refused before it reads anything behind it
    inf = math.inf

    def call(*, z=one, g=grid, ng=3, coef=good, corr=1, cfg=None, rescale=0.0, limit=inf, use_cfg=1, args=a):
        return lib.lt_sample_ode_multistep(one, z, None, one, g, ng, coef, corr, cfg, rescale, limit, use_cfg, 1,
                                           C.byref(args) if args is not None else None, None)

    def packed(*, hw=(C.c_int32 * 4)(16, 16, 16, 16), ng=3, coef=good, corr=1):
        return lib.lt_sample_ode_multistep_packed(one, one, hw, None, one, grid, ng, coef, corr, 1, 1, C.byref(a), None)

    def refused(rc, *words):
        msg = lib.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)

    refused(call(z=None), "lt_sample_ode_multistep: null argument")
    refused(call(g=None), "lt_sample_ode_multistep: null argument")
    refused(call(coef=None), "lt_sample_ode_multistep: null argument")
    refused(call(args=None), "lt_sample_ode_multistep: null argument")
    refused(call(ng=1), "lt_sample_ode_multistep:", "2 grid points")
    refused(call(corr=2), "lt_sample_ode_multistep:", "corrector 2 is not 0")
    refused(call(corr=-1), "lt_sample_ode_multistep:", "corrector -1 is not 0")
    refused(call(coef=nan), "lt_sample_ode_multistep:", "b[0] of interval 1 is not finite")
    refused(call(coef=early, corr=0), "lt_sample_ode_multistep:", "interval 0 names 2 slopes")
    refused(call(cfg=F(4.0, 4.0), use_cfg=0), "lt_sample_ode_multistep:", "guidance table with use_cfg = 0")
    refused(call(rescale=0.5, use_cfg=0), "lt_sample_ode_multistep:", "rule with use_cfg = 0")
    refused(packed(hw=None), "lt_sample_ode_multistep_packed: null argument")
    refused(packed(ng=1), "lt_sample_ode_multistep_packed:", "2 grid points")
    refused(packed(corr=2), "lt_sample_ode_multistep_packed:", "corrector 2")
    refused(packed(coef=nan), "lt_sample_ode_multistep_packed:", "not finite")
    # the op entry
    k = (C.c_void_p * 4)(64, 64, 64, 64)
    w = (C.c_float * 4)(0.5, 0.25, 0.0, 0.0)
    op = lib.lt_op_ode_multistep
    refused(op(one, k, 2, w, w, 1, one, one, 16, 2, None), "ode_multistep: state dtype")
    refused(op(one, k, 2, w, w, 2, one, one, 16, 1, None), "ode_multistep: has_corr 2")
    refused(op(None, k, 2, w, w, 1, one, one, 16, 1, None), "ode_multistep: null argument")
    refused(op(one, k, 2, w, w, 1, None, one, 16, 1, None), "ode_multistep: null argument (the corrector")
    refused(op(one, k, 0, w, w, 1, one, one, 16, 1, None), "ode_multistep: nslopes 0")
    refused(op(one, k, 5, w, w, 1, one, one, 16, 1, None), "ode_multistep: nslopes 5")
    refused(op(one, k, 1, w, w, 1, one, one, 16, 1, None), "ode_multistep: the weights name 2 slopes, 1 are given")
    refused(op(one, k, 2, w, (C.c_float * 4)(0.5, float("inf"), 0, 0), 0, None, one, 16, 1, None), "ode_multistep: weight 1 is not finite")
    refused(op(one, (C.c_void_p * 4)(64, 0, 0, 0), 2, w, w, 1, one, one, 16, 1, None), "ode_multistep: slope 1 of 2 is null")


def test_the_engine_layer_refuses_by_name_without_a_device():
    from lumina_t2x_amd.engine import DiTEngine
    with pytest.raises(_lib.LuminaLibError, match="multistep method 'ab4' not in"):
        DiTEngine._multistep_table([0.0, 0.5, 1.0], "ab4", 3, "sample_ode_multistep")
    with pytest.raises(_lib.LuminaLibError, match="at least 2 grid points"):
        DiTEngine._multistep_table([0.0], "ab2", 1, "sample_ode_multistep")
    with pytest.raises(_lib.LuminaLibError, match="sample_ode_masked: masked .* multistep method \\(abm3\\) is refused"):
        DiTEngine._refuse_masked_multistep("abm3", "sample_ode_masked")
    DiTEngine._refuse_masked_multistep("midpoint", "sample_ode_masked")
    tab, corr = DiTEngine._multistep_table([0.0, 0.25, 1.0], "abm2", 3, "x")
    assert tab.shape == (2, 8) and corr == 1 and DiTEngine._multistep_table([0.0, 0.25, 1.0], "ab3", 3, "x")[1] == 0


def test_sample_driver_takes_the_methods_under_both_option_names():
    from lumina_t2x_amd import sample as S
    p = S.build_parser()
    assert p.parse_args(["--ckpt", "c", "--solver", "abm2"]).sampling_method == "abm2"
    assert p.parse_args(["--ckpt", "c", "--sampling-method", "ab3"]).sampling_method == "ab3"
    assert p.parse_args(["--ckpt", "c"]).sampling_method == "euler"
