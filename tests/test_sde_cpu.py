"""CPU: SDE sampling inside the engine (lt_sample_sde / lt_op_sde_step) - the C ABI surface, the coefficient table the Python sampler hands
to the engine, and a torch restatement of what the engine computes (tests/sde_torch.py: ONE model evaluation per stage, table-driven
coefficients, stored noise) against the trajectory of the UNMODIFIED reference sampler (tests/golden/sde_imagenet_tiny.npz,
scripts/make_sde_golden.py)."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import integrators as I
from lumina_t2x_amd.transport import path
from oracle import synth
from oracle import variants_oracle as V

import sde_torch as ST

FORMS = ("SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing")


def test_header_declares_the_sde_calls_and_the_binding_matches():
    text = _lib.header_text()
    protos = dict(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    for name, n_args in (("lt_sample_sde", 13), ("lt_op_sde_step", 12)):
        assert name in protos, f"{name} is not declared in include/lumina_dit.h"
        assert len(protos[name].split(",")) == n_args
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name][1]) == n_args
    for k, v in {**_lib.SDE_METHODS, **{f"LAST_{k}": v for k, v in _lib.SDE_LAST_STEPS.items()}}.items():
        key = {"Euler": "LT_SDE_EULER", "Heun": "LT_SDE_HEUN", "LAST_None": "LT_SDE_LAST_NONE", "LAST_Mean": "LT_SDE_LAST_MEAN",
               "LAST_Tweedie": "LT_SDE_LAST_TWEEDIE", "LAST_Euler": "LT_SDE_LAST_EULER"}[k]
        assert re.search(r"#define %s %d\b" % (key, v), text), key
    assert re.search(r"#define LT_SDE_REC %d\b" % _lib.LT_SDE_REC, text)
    for name in ("EULER", "HEUN_XHAT", "HEUN_K1", "HEUN_OUT", "LAST_MEAN", "LAST_TWEEDIE", "LAST_EULER"):
        assert re.search(r"#define LT_SDE_OP_%s %d\b" % (name, getattr(_lib, "LT_SDE_OP_" + name)), text), name


def test_argument_errors_come_back_by_name_without_a_device():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.lt_sample_sde(None, None, None, None, None, None, 6, 0, 0, None, 1, None, None) != 0
    assert b"lt_sample_sde" in lib.lt_last_error() and b"null" in lib.lt_last_error()
    rec = (C.c_float * 8)(*([1.0] * 8))
    assert lib.lt_op_sde_step(99, None, None, None, None, None, None, None, rec, 8, 1, None) != 0
    assert b"unknown op" in lib.lt_last_error()
    assert lib.lt_op_sde_step(0, None, None, None, None, None, None, None, rec, 8, 1, None) != 0
    assert b"null" in lib.lt_last_error()


def _host_scalars(plan, form, norm, tvec, x):
    """the [B,1,1,1] tensors of one host-loop stage at the [B] time vector ``tvec`` -> first row's values"""
    r, sigma_t, d_sigma_t = plan._ratio_and_coeffs(x, tvec)
    var = sigma_t**2 - r * d_sigma_t * sigma_t
    D = plan.compute_diffusion(x, tvec, form=form, norm=norm)
    return [float(v.reshape(-1)[0]) for v in (tvec, r, var, D, torch.sqrt(2 * D))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("plan_cls", [path.ICPlan, path.GVPCPlan, path.VPCPlan])
def test_table_holds_the_scalars_the_plan_gives_on_a_batch_time_vector(plan_cls, dtype):
    """every plan x every form the host loop accepts ("constant" fails in its th.sqrt) x both methods: each record of sde_table equals what
    the loop's own expressions give on a [B] time vector of the state dtype - NaN / inf included (SBDM at t = 0 on the Linear / GVP paths)"""
    plan = plan_cls()
    B, norm = 3, 0.7
    x = torch.zeros(B, 4, 8, 8, dtype=dtype)
    for t0, t1 in ((0.0, 0.96), (1e-3, 0.999)):
        t = torch.linspace(t0, t1, 7)
        dt = t[1] - t[0]
        for form in FORMS:
            for method, stages in (("Euler", 1), ("Heun", 2)):
                for last_step in (None, "Mean", "Tweedie", "Euler"):
                    steps, last = I.sde_table(plan, form, norm, t, dt, method, x, last_step, 0.04, t1)
                    assert steps.shape == (6 * stages, _lib.LT_SDE_REC) and steps.dtype == torch.float32
                    for i, ti in enumerate(t[:-1]):
                        tvec = torch.ones(B).to(x) * ti
                        for k in range(stages):
                            want = _host_scalars(plan, form, norm, tvec if k == 0 else tvec + dt, x)
                            want += [float(dt), float(torch.sqrt(dt)), float(0.5 * dt)]
                            got = steps[i * stages + k].tolist()
                            assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(got, want)), (form, method, i, k, got, want)
                    if last_step is None:
                        assert last is None
                        continue
                    ts = torch.ones(B) * t1
                    want = _host_scalars(plan, form, norm, ts, x)[:4]
                    a, s = plan.compute_alpha_t(ts)[0][0], plan.compute_sigma_t(ts)[0][0]
                    want += [float(torch.tensor(0.04, dtype=torch.float32)), float(a.to(dtype)), float((s**2) / a), 0.0]
                    got = last.tolist()
                    assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(got, want)), (form, last_step, got, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_score_and_drift_from_the_table_equal_the_plans_own(dtype):
    """(r v - x) / var with the table's r, var is ICPlan.get_score_from_velocity, and v + D score is Sampler's sde_drift evaluated with ONE
    model output - bit for bit, at both state dtypes"""
    torch.manual_seed(3)
    B = 2
    x, v = torch.randn(B, 4, 8, 8).to(dtype), torch.randn(B, 4, 8, 8).to(dtype)
    for ptype in ("Linear", "GVP", "VP"):
        tr = create_transport(ptype, "velocity", None, None, None)
        plan = tr.path_sampler
        t = torch.linspace(0.05, 0.9, 5)
        for form in FORMS:
            steps, _ = I.sde_table(plan, form, 0.7, t, t[1] - t[0], "Euler", x)
            sde_drift, _ = Sampler(tr)._sde_terms(form, 0.7)
            for i, ti in enumerate(t[:-1]):
                c = ST.Stage(steps[i], x)
                tvec = torch.ones(B).to(x) * ti
                assert torch.equal((c.r * v - x) / c.var, plan.get_score_from_velocity(v, x, tvec))
                assert torch.equal(ST.drift(x, v, c), sde_drift(x, tvec, lambda xx, tt: v))


def test_restated_engine_loop_reproduces_the_reference_trajectory(golden_dir):
    """fp32, oracle forward: one evaluation per stage + table coefficients + the stored draws give the reference's states (<= 1e-5 rel-L2
    at every stored step, last step included), with half the reference's evaluations"""
    g = np.load(os.path.join(golden_dir, "sde_imagenet_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    z, y = torch.from_numpy(g["z"]), torch.from_numpy(g["y"])
    cases, paths = json.loads(str(g["cases"])), json.loads(str(g["paths"]))
    n = int(g["num_steps"])
    assert set(cases) == {"euler_sigma_mean", "heun_sbdm_tweedie"}

    def model_fn(x, t):
        return V.imagenet_forward_with_cfg(sd, cfg, x, t, y, float(g["cfg_scale"]))

    for name, kw in cases.items():
        tr = create_transport(paths[name], "velocity", None, None, None)
        fn = Sampler(tr).sample_sde(num_steps=n, **kw)
        solver = fn.solver
        steps, last = I.sde_table(tr.path_sampler, kw["diffusion_form"], kw["diffusion_norm"], solver.t, solver.dt, kw["sampling_method"], z,
                                  kw["last_step"], kw["last_step_size"], solver.engine_plan["t1"])
        xs, fin = ST.sample(model_fn, z, torch.from_numpy(g[f"{name}_noise"]), steps, last, kw["sampling_method"], kw["last_step"])
        stages = 2 if kw["sampling_method"] == "Heun" else 1
        assert ST.sample.nfe == (n - 1) * stages + 1
        ref = torch.from_numpy(g[f"{name}_ref"])
        errs = [float((a - b).norm() / b.norm()) for a, b in zip(xs, ref)]
        errs.append(float((fin - torch.from_numpy(g[f"{name}_ref_last"])).norm() / torch.from_numpy(g[f"{name}_ref_last"]).norm()))
        print(name, "rel-L2 per stored step:", " ".join(f"{e:.2e}" for e in errs))
        assert len(errs) == n and max(errs) <= 1e-5, (name, errs)


def test_host_loop_is_kept_for_what_the_engine_does_not_serve():
    """score / noise prediction, the "constant" form, a CPU state and any callable that is not an engine-backed bound method stay on the
    host loop; use_engine = False switches back by hand"""
    x = torch.zeros(2, 4, 8, 8)
    for pred, form, want_plan_ok in (("velocity", "sigma", True), ("score", "sigma", False), ("noise", "sigma", False), ("velocity", "constant", False)):
        fn = Sampler(create_transport("Linear", pred, None, None, None)).sample_sde(diffusion_form=form, num_steps=4)
        s = fn.solver
        assert s.use_engine is True and s._engine_target(x, lambda a, b: a) is None
        ep = s.engine_plan
        assert (ep["velocity"] and ep["form"] in I._SDE_TENSOR_FORMS) is want_plan_ok
    fn = Sampler(create_transport("Linear", "velocity", None, None, None)).sample_sde(diffusion_form="constant", num_steps=4)
    with pytest.raises(TypeError):  # the reference's own th.sqrt(2 * float), unchanged
        fn(x, lambda a, b: a)
