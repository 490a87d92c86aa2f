"""CPU: step caching - the controller in Python floats on hand-made sequences, the argument checks, the table of combinations
refused by name, and the float64 restatements the GPU tests compare with."""
import math

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd.transport import cache as TC
from lumina_t2x_amd.transport.mini import ODE

import exact_cache as X


def _run(rels, thr, coef=TC.IDENTITY, s0=1.0):
    """the controller over evaluations whose indicator is S1 = rel * s0, S0 = s0; returns [(rel, acc, ran)]"""
    ctl = TC.CacheController(len(rels), thr, coef)
    return [ctl.step(j, r * s0, s0) for j, r in enumerate(rels)]


def test_first_and_last_always_run_and_read_nothing():
    out = _run([0.0] * 6, 1e30)
    assert [o[2] for o in out] == [True, False, False, False, False, True]
    assert out[0][:2] == (0.0, 0.0) and out[-1][0] == 0.0
    ctl = TC.CacheController(3, 5.0)
    assert ctl.step(0, float("nan"), float("nan")) == (0.0, 0.0, True)  # the sums of the first evaluation are not looked at
    assert not ctl.reads(0) and ctl.reads(1) and not ctl.reads(2)
    assert [o[2] for o in _run([9.0], 1e30)] == [True] and [o[2] for o in _run([9.0, 9.0], 1e30)] == [True, True]


def test_accumulator_resets_whenever_the_stack_runs():
    out = _run([0, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0], 0.625)
    # acc: .25 .5 .75(run) .25 .5 .75(run)
    assert [o[2] for o in out] == [True, False, False, True, False, False, True, True]
    assert [o[1] for o in out] == [0.0, 0.25, 0.5, 0.75, 0.25, 0.5, 0.75, 0.0]
    # acc == thr exactly runs: the rule is not (acc < thr)
    assert [o[2] for o in _run([0, 0.5, 0.5, 0], 1.0)] == [True, False, True, True]


def test_threshold_zero_always_runs_and_nan_runs():
    assert all(o[2] for o in _run([0, 0.0, 0.5, 0.0, 0], 0.0))
    out = _run([0, float("nan"), 0.1, 0], 10.0)
    assert out[1][2] is True and math.isnan(out[1][1]) and out[2][:2] == (0.1, 0.1) and out[2][2] is False  # NaN is not < thr; then acc is 0 again


def test_s0_zero_runs_and_adds_nothing():
    ctl = TC.CacheController(5, 10.0)
    ctl.step(0)
    assert ctl.step(1, 0.3, 1.0) == (0.3, 0.3, False)
    assert ctl.step(2, 0.0, 0.0) == (math.inf, 0.3, True) and ctl.acc == 0.0
    assert ctl.step(3, 0.2, 1.0) == (0.2, 0.2, False)


def test_polynomial_is_horner_highest_power_first():
    c = (2.0, -3.0, 0.5, 7.0, -1.0)
    r = 0.37
    assert TC.poly(r, c) == (((2.0 * r + -3.0) * r + 0.5) * r + 7.0) * r + -1.0
    assert TC.poly(r, TC.IDENTITY) == r and TC.poly(r, (0, 0, 0, 0, 4.0)) == 4.0
    out = _run([0, r, r, 0], 100.0, c)
    assert out[1][1] == TC.poly(r, c) and out[2][1] == TC.poly(r, c) + TC.poly(r, c)


def test_argument_checks_refuse_by_name():
    assert TC.check_cache_args(0.1) == (float(torch.tensor(0.1, dtype=torch.float32)), TC.IDENTITY)
    for bad, word in ((-0.1, ">= 0"), (float("nan"), ">= 0"), ("x", "not a number"), (None, "not a number")):
        with pytest.raises(ValueError, match=word):
            TC.check_cache_args(bad)
    for bad, word in (((1, 2, 3), "five numbers"), ((1, 2, 3, 4, float("inf")), "finite"), (3.0, "five numbers")):
        with pytest.raises(ValueError, match=word):
            TC.check_cache_args(0.1, bad)
    assert [TC.check_cache_method(m) for m in ("euler", "midpoint", "rk4")] == [1, 2, 4]
    for m, word in (("ab2", "multistep"), ("abm3", "multistep"), ("dopri5", "adaptive"), ("heun2", "fixed-grid")):
        with pytest.raises(ValueError, match=word):
            TC.check_cache_method(m)


REFUSED = [("cfg_interval", (0.1, 0.8), "cfg_interval"), ("cfg_schedule", "linear", "cfg_schedule"), ("cfg_table", [4.0], "cfg_table"),
           ("cfg_rescale", 0.5, "cfg_rescale"), ("cfg_norm_limit", 2.0, "cfg_norm_limit"), ("cfg_reuse", [0, 1], "cfg_reuse"),
           ("slg", [1], "skip-layer"), ("mask", torch.ones(1), "mask"), ("packed", True, "packed batch")]


@pytest.mark.parametrize("name,value,word", REFUSED)
def test_combinations_refused_by_name(name, value, word):
    with pytest.raises(ValueError, match=word):
        TC.refuse_with_teacache("euler", **{name: value})
    assert set(TC.REFUSED_WITH) == {r[0] for r in REFUSED}


def test_switched_off_options_pass_and_methods_are_refused():
    TC.refuse_with_teacache("rk4", cfg_interval=None, cfg_schedule=None, cfg_table=None, cfg_rescale=0.0, cfg_norm_limit=math.inf, cfg_reuse=0,
                            slg=None, mask=None, packed=False)
    TC.refuse_with_teacache("euler", slg=(), cfg_reuse=False)
    with pytest.raises(ValueError, match="multistep"):
        TC.refuse_with_teacache("abm2")
    with pytest.raises(ValueError, match="adaptive"):
        TC.refuse_with_teacache("dopri5")
    with pytest.raises(TypeError, match="unknown option"):
        TC.refuse_with_teacache("euler", bogus=1)


def test_front_end_refuses_a_model_that_is_not_engine_backed_and_the_combinations():
    o = ODE(5, "euler", 4)
    z = torch.zeros(2, 4, 8, 8)
    with pytest.raises(TypeError, match="engine-backed"):
        o.sample(z, lambda x, t, **kw: x, teacache=0.1)
    with pytest.raises(ValueError, match="cfg_reuse"):
        o.sample(z, lambda x, t, **kw: x, teacache=0.1, cfg_reuse=[0, 1, 0, 1])
    with pytest.raises(ValueError, match="packed batch"):
        o.sample([z[0], z[1]], lambda x, t, **kw: x, teacache=0.1)
    with pytest.raises(ValueError, match="multistep"):
        ODE(5, "ab2", 4).sample(z, lambda x, t, **kw: x, teacache=0.1)
    with pytest.raises(TypeError, match="engine-backed"):
        TC.sample_teacache(object(), z, o.t, "euler", threshold=0.1)


def test_driver_arguments():
    from lumina_t2x_amd import sample as S
    base = ["--ckpt", "x"]
    p = S.build_parser()
    assert S.step_cache(p.parse_args(base)) == {}
    got = S.step_cache(p.parse_args(base + ["--teacache", "0.25", "--teacache_coefficients", "1", "2", "3", "4", "5"]))
    assert got == dict(teacache=0.25, teacache_coefficients=(1.0, 2.0, 3.0, 4.0, 5.0))
    for extra, word in ((["--cfg_interval", "0.1", "0.8"], "cfg_interval"), (["--cfg_schedule", "cosine"], "cfg_schedule"),
                        (["--cfg_rescale", "0.5"], "cfg_rescale"), (["--cfg_norm_limit", "2"], "cfg_norm_limit"), (["--cfg_reuse", "2"], "cfg_reuse"),
                        (["--cfg_reuse_per_step"], "cfg_reuse"), (["--slg_layers", "1"], "skip-layer"), (["--solver", "abm2"], "multistep"),
                        (["--solver", "dopri5"], "adaptive")):
        with pytest.raises(SystemExit, match=word):
            S.step_cache(p.parse_args(base + ["--teacache", "0.1"] + extra))
    with pytest.raises(SystemExit, match=">= 0"):
        S.step_cache(p.parse_args(base + ["--teacache", "-1"]))
    with pytest.raises(SystemExit, match="needs --teacache"):
        S.step_cache(p.parse_args(base + ["--teacache_coefficients", "0", "0", "0", "1", "0"]))


def test_restatements_the_gpu_tests_compare_with():
    a, b = X.edge_operands(64, 3)
    r = X.ref_store(a, b)
    f = lambda v: float(v)  # noqa: E731
    assert f(r[0]) == 0.0 and f(r[1]) == 2.0 and f(r[10]) == 1.015625  # 1 + 2^-7 + 2^-8: a tie, up to the even neighbour
    x = X.ref_apply_x(a, b)
    assert f(x[7]) == 1.0 and f(x[9]) == 1.015625 and f(x[10]) == 1.0  # the ties go to the even neighbour on both sides
    assert math.isinf(f(x[14])) and f(x[15]) == 0.0 and math.isinf(f(x[18])) and math.isinf(f(x[17]))  # (the last tie's even neighbour is inf)
    assert X.bits(x[3:7]).tolist() == [0, 0, -32768, 0]  # +0 + -0 = +0, -0 + -0 = -0
    ia, ib = X.integer_operands(4096, 5)
    s1, s0 = X.ref_sums(ia, ib)
    assert s1 == float((ia.long() - ib.long()).abs().sum()) and s0 == float(ib.long().abs().sum())
    assert X.sum_bound(64) == 64 * 2.0 ** -53 and X.rel_bound(64) > 2 * X.sum_bound(64)
    assert X.chain_depth(64) == 30 and X.chain_depth(8 * 512 * 256 + 8) == 38
    assert TC.indicator_sums(ia, ib) == (s1, s0)
