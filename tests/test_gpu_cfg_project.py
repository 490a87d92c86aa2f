"""GPU: projected guidance, APG and CFG-Zero* - lt_sample_ode_cfg_project / lt_forward_cfg_project.  Everything but the sums is exact.

* kernels: the partial sums of lt_op_guidance_project_stats equal torch's float64 sums within ``n 2^-52 sum |term|`` (every partial is a float64
  sum of at most n terms in some order; so is torch's), nothing behind them is written, and APG's momentum words equal the definition's bit for
  bit from a non-zero ``m_prev``; lt_op_unpatchify_cfg_project equals ``transport.guidance.guided_project`` word for word, coefficients
  included, when the definition is handed the device partials added on the host in slice order (``sums=``) - so the comparison does not hang on
  the order of a float64 summation; the dup form and the channels past ``ch`` equal lt_op_unpatchify_cfg_dev;
* loop: the engine's trajectory equals the host loop ``sample_cfg_project`` around the same model at every slot - the host loop reduces with
  torch, as ``sample_cfg_rule`` does; where a coefficient word were ever to differ on these fixed seeds the assertion prints the float64 pair;
* state: the momentum starts every trajectory at zero, continues over ``keep_momentum`` calls, is forgotten by a new prompt;
* graph path: two keys whatever the table and the parameters hold; the schedule and the rule call are what they were;
* a class-conditional family and Flag-DiT through ``ODE.sample``; refusals by name; the ``sample.py`` driver."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import EngineLimits
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

from gpu_util import P, lib, stream
from test_gpu_cfg_rule import KERNEL_SHAPES, _bits, _f32, _rows
from test_gpu_cfg_schedule import _grid, _tables
from test_gpu_sde import _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
INF = math.inf
APG, ZERO = _lib.LT_PROJECT_APG, _lib.LT_PROJECT_ZERO_STAR
_CACHE = {}


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
def _m_prev(half, ch, H, W, seed):
    return torch.randn(half, ch, H, W, generator=torch.Generator().manual_seed(seed)).mul(2).to("cuda")


def _stats(L, rows, ld, B, H, W, ch, ws, form, par, mom, pad=0, sentinel=0.0):
    S = L.lt_op_guidance_slices()
    half = B // 2
    parts = torch.full((half * S * 3 + pad,), sentinel, dtype=torch.float64, device="cuda")
    rc = L.lt_op_guidance_project_stats(P(rows), ld, B, 8, H, W, 2, ch, ws, form, P(par) if par is not None else None,
                                        P(mom) if mom is not None else None, P(parts), stream())
    assert rc == 0, L.lt_last_error()
    return parts


def _host_sums(parts, half, S, count):
    """the device partials added on the host in slice order, as the closing kernel adds them: a list of per-sample tuples"""
    p = parts[: half * S * 3].view(half, S, 3).cpu().tolist()
    out = []
    for b in range(half):
        acc = [0.0, 0.0, 0.0]
        for s in range(S):
            for k in range(3):
                acc[k] += p[b][s][k]
        out.append(tuple(acc[:count]))
    return out


@pytest.mark.parametrize("eol", [0, 1], ids=["grid", "eol"])
@pytest.mark.parametrize("B,H,W", KERNEL_SHAPES)
def test_stats_partials_sum_to_the_float64_sums_momentum_words_are_exact_and_nothing_else_is_written(B, H, W, eol):
    L = lib()
    S = L.lt_op_guidance_slices()
    half = B // 2
    rows, o, stride, ld = _rows(B, H, W, eol, seed=140 + B + H + eol)
    ws = stride if eol else 0
    sentinel = -7.25
    for ch in (3, 4):
        n = ch * H * W
        c, u = o[:half, :ch], o[half:, :ch]
        cd, ud = c.double().reshape(half, -1), u.double().reshape(half, -1)
        for beta in (0.0, -0.5, 0.75):
            par = torch.tensor([4.0, 0.5, beta, INF], dtype=torch.float32, device="cuda")
            prev = _m_prev(half, ch, H, W, seed=7 + ch)
            mom = torch.full((half * n + 32,), sentinel, dtype=torch.float32, device="cuda")
            mom[: half * n] = prev.reshape(-1)
            parts = _stats(L, rows, ld, B, H, W, ch, ws, APG, par, mom, pad=16, sentinel=sentinel)
            assert bool((parts[half * S * 3:] == sentinel).all()) and not bool((parts[: half * S * 3] == sentinel).any())
            assert bool((mom[half * n:] == sentinel).all())
            _, _, m = G.guided_project(o, 4.0, ch, "apg", eta=0.5, momentum=beta, m_prev=prev)
            assert torch.equal(_bits(mom[: half * n]), _bits(m.reshape(-1))), (B, H, W, eol, ch, beta)
            if beta != 0.0:
                assert not torch.equal(m, (c - u).float())
            got = parts[: half * S * 3].view(half, S, 3)
            if n < S:  # one element per slice: the slices behind the last element hold zeros
                assert bool((got[:, n:] == 0).all())
            got = got.sum(1).cpu()
            md = m.double().reshape(half, -1)
            for k, term in enumerate((md * md, md * cd, cd * cd)):
                want, mag = term.sum(1).cpu(), term.abs().sum(1).cpu()
                err = (got[:, k] - want).abs()
                print(f"apg B {B} {H}x{W} eol {eol} ch {ch} beta {beta} sum {k}: err {err.tolist()} bound {(n * 2.0 ** -52 * mag).tolist()}")
                assert bool((err <= n * 2.0 ** -52 * mag).all()), (ch, beta, k, err.tolist(), mag.tolist())
        parts = _stats(L, rows, ld, B, H, W, ch, ws, ZERO, None, None, pad=16, sentinel=sentinel)
        assert bool((parts[half * S * 3:] == sentinel).all()) and not bool((parts[: half * S * 3] == sentinel).any())
        got = parts[: half * S * 3].view(half, S, 3).sum(1).cpu()
        assert bool((got[:, 2] == 0).all())
        for k, term in enumerate((cd * ud, ud * ud)):
            want, mag = term.sum(1).cpu(), term.abs().sum(1).cpu()
            err = (got[:, k] - want).abs()
            print(f"zero* B {B} {H}x{W} eol {eol} ch {ch} sum {k}: err {err.tolist()} bound {(n * 2.0 ** -52 * mag).tolist()}")
            assert bool((err <= n * 2.0 ** -52 * mag).all()), (ch, k, err.tolist(), mag.tolist())


@pytest.mark.parametrize("eol", [0, 1], ids=["grid", "eol"])
@pytest.mark.parametrize("B,H,W", KERNEL_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_project_kernel_equals_guided_project_word_for_word(dtype, B, H, W, eol):
    L = lib()
    S = L.lt_op_guidance_slices()
    Cc, half = 4, B // 2
    rows, o, stride, ld = _rows(B, H, W, eol, seed=160 + B + H + eol)
    n = B * Cc * H * W
    code = _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32
    sentinel = 1.5
    ws = stride if eol else 0

    def dev(scale, ch, dup):
        out = torch.full((n + 64,), sentinel, dtype=dtype, device="cuda")
        sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
        rc = L.lt_op_unpatchify_cfg_dev(P(rows), ld, P(out), code, B, Cc, 8, H, W, 2, 1, P(sc), ch, ws, dup, stream())
        assert rc == 0, L.lt_last_error()
        return out

    def project(form, scale, ch, eta=1.0, beta=0.0, r=INF, prev=None, dup=0):
        out = torch.full((n + 64,), sentinel, dtype=dtype, device="cuda")
        ncoef = half * (2 if form == APG else 1)
        coef = torch.full((ncoef + 8,), sentinel, dtype=torch.float32, device="cuda")
        par = torch.tensor([scale, eta, beta, r], dtype=torch.float32, device="cuda")
        mom = (prev.clone() if prev is not None else torch.zeros(half, ch, H, W, device="cuda")).contiguous()
        parts = torch.zeros(half * S * 3, dtype=torch.float64, device="cuda")
        if not dup:
            parts = _stats(L, rows, ld, B, H, W, ch, ws, form, par, mom)
        rc = L.lt_op_unpatchify_cfg_project(P(rows), ld, P(out), code, B, Cc, 8, H, W, 2, 1, P(par), ch, ws, dup, form, P(parts), P(par), P(mom),
                                            P(coef), stream())
        assert rc == 0, L.lt_last_error()
        assert bool((out[n:] == sentinel).all()) and bool((coef[ncoef:] == sentinel).all())
        return out, coef[:ncoef], _host_sums(parts, half, S, 3 if form == APG else 2)

    for ch in (3, 4):
        prev = _m_prev(half, ch, H, W, seed=11 + ch)
        # r between the samples' |m|: the definition's own sums say which samples it clips
        info = []
        G.guided_project(o, 4.0, ch, "apg", momentum=0.75, m_prev=prev, parts=info)
        norms = [math.sqrt(p[0]) for p in info]
        if half > 1:
            assert min(norms) * 1.05 < max(norms), norms
            r_mid = _f32(math.sqrt(min(norms) * max(norms)))
        else:
            r_mid = _f32(norms[0] * 0.5)
        for scale in (0.0, 4.0, 7.5, -1.5):
            for eta in (0.0, 0.5, 1.0):
                for beta, r in ((0.0, INF), (0.75, r_mid), (-0.5, _f32(max(norms) * 4.0))):
                    tag = (dtype, B, H, W, eol, ch, scale, eta, beta, r)
                    got, coef, sums = project(APG, scale, ch, eta, beta, r, prev)
                    info = []
                    want, cw, _ = G.guided_project(o, scale, ch, "apg", eta=eta, momentum=beta, norm_threshold=r, m_prev=prev, sums=sums, parts=info)
                    if r == r_mid and half > 1:
                        assert any(p[3] < 1.0 for p in info) and any(p[3] == 1.0 for p in info), tag + (info,)
                    if r == r_mid and half == 1:
                        assert info[0][3] < 1.0, tag + (info,)
                    if r > r_mid:
                        assert all(p[3] == 1.0 for p in info), tag + (info,)
                    assert torch.equal(_bits(coef), _bits(cw.reshape(-1))), tag + (coef.tolist(), cw.tolist(), sums)
                    assert torch.equal(_bits(got[:n]), _bits(want.to(dtype).reshape(-1))), tag
            got, coef, sums = project(ZERO, scale, ch)
            want, cw, _ = G.guided_project(o, scale, ch, "zero_star", sums=sums)
            assert torch.equal(_bits(coef), _bits(cw)), (dtype, B, H, W, eol, ch, scale, coef.tolist(), cw.tolist(), sums)
            assert torch.equal(_bits(got[:n]), _bits(want.to(dtype).reshape(-1))), (dtype, B, H, W, eol, ch, scale)
            # the channels past ch pass through row by row, as in lt_op_unpatchify_cfg_dev
            if ch < Cc:
                plain = dev(scale, ch, 0)[:n].view(B, Cc, H, W)
                assert torch.equal(_bits(got[:n].view(B, Cc, H, W)[:, ch:]), _bits(plain[:, ch:]))
        for form in (APG, ZERO):
            got, coef, _ = project(form, 4.0, ch, 0.5, 0.75, 1.0, prev, dup=1)
            assert torch.equal(_bits(got), _bits(dev(4.0, ch, 1))) and bool((coef == sentinel).all()), (dtype, B, H, W, eol, ch, form)


# ---- loop ----------------------------------------------------------------------------------------------------------------------------
def _next(golden_dir):
    if "next" not in _CACHE:
        model, z, kw = _model(golden_dir, "next")
        _CACHE["next"] = (model, kw)
    return _CACHE["next"]


def _apg_threshold(model, z, tgrid, table, method, cf, cm, step_kw):
    """a norm threshold between the smallest and the largest |m| the unclipped trajectory meets: it engages at some stage, not at every one"""
    parts = []
    G.sample_cfg_project(model, z, tgrid, table, method, apg=dict(eta=0.5, momentum=-0.5), parts=parts, cap_feats=cf, cap_mask=cm, **step_kw)
    norms = sorted(math.sqrt(p[0]) for p in parts)
    return _f32(norms[len(norms) // 2] * 0.999)


def _same_coefficients(fa, fb, parts_a, tag):
    """the coefficient words of two runs; a difference prints the float64 sums behind it"""
    assert len(fa) == len(fb), tag
    for k, (x, y) in enumerate(zip(fa, fb)):
        assert torch.equal(_bits(x), _bits(y)), tag + (k, x.tolist(), y.tolist(), parts_a[k * x.shape[0]: (k + 1) * x.shape[0]])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    step_kw = dict(proportional_attn=True, base_seqlen=16)
    tgrid = _grid(method)
    st = STAGES[method]
    n = (len(tgrid) - 1) * st
    g = torch.Generator().manual_seed(16)
    for B, H, W in ((2, 16, 16), (4, 16, 24)):
        Bh = B // 2
        z = torch.randn(Bh, 4, H, W, generator=g).to("cuda", dtype).repeat(2, 1, 1, 1)
        cf, cm = (cap, cmask) if B == 2 else (torch.cat([cap, cap.flip(0)]), torch.cat([cmask, cmask.flip(0)]))
        t0 = torch.full((B,), 0.25, device="cuda")
        model.forward_with_cfg(z, t0, cf, cm, 4.0, **step_kw)  # the flags a plain forward reads
        tabs = _tables(tgrid, method)
        for name in ("interval", "ramp"):
            table = tabs[name]
            tag = (method, dtype, B, name)
            G_, C_ = int((table != 1).sum()), int((table == 1).sum())
            off = model.sample_ode_cfg_schedule(z, tgrid, table, cf, cm, method=method, return_trajectory=True, **step_kw)
            eng = model._engine
            # APG: momentum, a threshold that engages at some stages, a damped parallel part
            apg = dict(eta=0.5, momentum=-0.5, norm_threshold=_apg_threshold(model, z, tgrid, table, method, cf, cm, step_kw))
            got = model.sample_ode_cfg_schedule(z, tgrid, table, cf, cm, method=method, return_trajectory=True, apg=apg, **step_kw)
            assert eng.last_nfe() == n and eng.last_eval_rows() == B * G_ + Bh * C_, tag + (eng.last_nfe(), eng.last_eval_rows())
            final = model.sample_ode_cfg_schedule(z, tgrid, table, cf, cm, method=method, apg=apg, **step_kw)
            parts = []
            want = G.sample_cfg_project(model, z, tgrid, table, method, apg=apg, parts=parts, cap_feats=cf, cap_mask=cm, **step_kw)
            assert len(parts) == G_ * Bh and any(p[3] < 1.0 for p in parts), tag + (parts,)  # the norm threshold engages at some stage
            assert got.shape == want.shape == (len(tgrid),) + tuple(z.shape) and got.dtype == dtype, tag
            assert bool(torch.isfinite(want.float()).all()), tag
            for i in range(len(tgrid)):
                assert torch.equal(got[i], want[i]), tag + ("apg", i, int((got[i] != want[i]).sum()), parts)
            assert torch.equal(final, got[-1]) and not torch.equal(got[-1], off[-1]), tag
            # CFG-Zero*, with one interval of zero velocity
            for K in (0, 1):
                gz = int((table[K * st:] != 1).sum())
                cz = int((table[K * st:] == 1).sum())
                got = model.sample_ode_cfg_schedule(z, tgrid, table, cf, cm, method=method, return_trajectory=True, zero_star=True, zero_init=K, **step_kw)
                assert eng.last_nfe() == n - K * st and eng.last_eval_rows() == B * gz + Bh * cz, tag + (K, eng.last_nfe(), eng.last_eval_rows())
                parts, calls = [], []
                want = G.sample_cfg_project(model, z, tgrid, table, method, zero_star=True, zero_init=K, parts=parts, calls=calls, cap_feats=cf,
                                            cap_mask=cm, **step_kw)
                assert calls == [n - K * st] and len(parts) == gz * Bh, tag
                for i in range(len(tgrid)):
                    assert torch.equal(got[i], want[i]), tag + ("zero*", K, i, int((got[i] != want[i]).sum()), parts)
                for i in range(K + 1):
                    assert torch.equal(got[i], z), tag
                assert not torch.equal(got[-1], off[-1]), tag
        # one evaluation: guided_project on the model's output of all rows
        o = model.forward(torch.cat([z[:Bh]] * 2), t0, cf, cm)
        for w in (4.0, 1.0):
            want, _, _ = G.guided_project(o, w, 3, "apg", eta=0.25, norm_threshold=2.0)
            got = model.forward_with_cfg_project(z, t0, cf, cm, w, apg=dict(eta=0.25, norm_threshold=2.0), **step_kw)
            assert got.dtype == dtype and torch.equal(got, want), (method, dtype, B, w)
            want, _, _ = G.guided_project(o, w, 3, "zero_star")
            got = model.forward_with_cfg_project(z, t0, cf, cm, w, zero_star=True, **step_kw)
            assert got.dtype == dtype and torch.equal(got, want), (method, dtype, B, w)
        assert torch.equal(model.forward_with_cfg_project(z, t0, cf, cm, 4.0, **step_kw), model.forward_with_cfg(z, t0, cf, cm, 4.0, **step_kw))


# ---- state ---------------------------------------------------------------------------------------------------------------------------
def test_momentum_starts_at_zero_continues_on_request_and_is_forgotten_by_a_new_prompt(golden_dir):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    step_kw = dict(proportional_attn=True, base_seqlen=16)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(21)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    z2 = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(22)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    t0, t1 = torch.full((2,), 0.25, device="cuda"), torch.full((2,), 0.5, device="cuda")
    plain = model.forward_with_cfg(z, t0, cap, cmask, 4.0, **step_kw)
    eng, L = model._engine, lib()
    tgrid = _grid("midpoint")
    table = _tables(tgrid, "midpoint")["ramp"]
    apg = dict(eta=0.5, momentum=0.75, norm_threshold=INF)
    # the same trajectory twice: the momentum the first call left plays no part in the second
    a = model.sample_ode_cfg_schedule(z, tgrid, table, cap, cmask, method="midpoint", return_trajectory=True, apg=apg, **step_kw)
    b = model.sample_ode_cfg_schedule(z, tgrid, table, cap, cmask, method="midpoint", return_trajectory=True, apg=apg, **step_kw)
    assert torch.equal(a, b)
    # two evaluations that share a momentum are two steps of the definition
    o1 = model.forward(torch.cat([z[:1]] * 2), t0, cap, cmask)
    o2 = model.forward(torch.cat([z2[:1]] * 2), t1, cap, cmask)
    w1, _, m1 = G.guided_project(o1, 4.0, 3, "apg", eta=0.5, momentum=0.75)
    w2, _, m2 = G.guided_project(o2, 3.0, 3, "apg", eta=0.5, momentum=0.75, m_prev=m1)
    fresh2, _, _ = G.guided_project(o2, 3.0, 3, "apg", eta=0.5, momentum=0.75)
    assert not torch.equal(w2, fresh2)
    g1 = model.forward_with_cfg_project(z, t0, cap, cmask, 4.0, apg=apg, **step_kw)
    # a plain guided evaluation in between returns what it returned before, and leaves the momentum alone
    assert torch.equal(model.forward_with_cfg(z, t0, cap, cmask, 4.0, **step_kw), plain)
    g2 = model.forward_with_cfg_project(z2, t1, cap, cmask, 3.0, apg=apg, keep_momentum=True, **step_kw)
    assert torch.equal(g1, w1) and torch.equal(g2, w2)
    assert torch.equal(model.forward_with_cfg_project(z2, t1, cap, cmask, 3.0, apg=apg, **step_kw), fresh2)  # keep_momentum off: from zero
    # a new prompt forgets the momentum: refused by name, out untouched
    eng.prepare_prompt(cap.clone(), cmask.clone())  # (another prompt object: the same one would be a cache hit on the Python side)
    out = torch.full_like(z, float("nan"))
    sa = eng._step_args(z, 4.0, 1.0, 1.0, 16, True)
    rc = L.lt_forward_cfg_project(eng.handle, P(z), P(t0), P(out), APG, 0.5, 0.75, INF, 1, C.byref(sa), stream())
    msg = L.lt_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "lt_forward_cfg_project:" in msg and "no stored momentum" in msg and bool(torch.isnan(out).all()), (rc, msg)
    # ... and so is another shape
    model.forward_with_cfg_project(z, t0, cap, cmask, 4.0, apg=apg, **step_kw)
    zw = torch.randn(1, 4, 16, 24, generator=torch.Generator().manual_seed(23)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    outw = torch.full_like(zw, float("nan"))
    sa = eng._step_args(zw, 4.0, 1.0, 1.0, 16, True)
    rc = L.lt_forward_cfg_project(eng.handle, P(zw), P(t0), P(outw), APG, 0.5, 0.75, INF, 1, C.byref(sa), stream())
    msg = L.lt_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "lt_forward_cfg_project:" in msg and "another shape" in msg and bool(torch.isnan(outw).all()), (rc, msg)
    assert torch.equal(model.forward_with_cfg(z, t0, cap, cmask, 4.0, **step_kw), plain)


# ---- graph keys ----------------------------------------------------------------------------------------------------------------------
def test_graph_path_replays_two_keys_and_leaves_the_schedule_and_the_rule_call_what_they_were(golden_dir):
    model, _, kw = _model(golden_dir, "next")  # a fresh engine: no key has been used
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    step_kw = dict(proportional_attn=True, base_seqlen=16)
    H, W = 50, 82  # 25 x 41 = 1025 tokens: the smallest latent whose B' = 1 evaluation has more than 1024 rows
    tgrid = _grid("midpoint")
    table = torch.tensor([1.0, 2.0, 1.0, 3.0, 3.5, 1.0, 4.5, 5.0])
    G_, C_ = 5, 3
    z = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(18)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), cap, cmask, 4.0, **step_kw)  # engine, weights, prompt
    eng = model._engine
    run = lambda **k: model.sample_ode_cfg_schedule(z, tgrid, table, cap, cmask, method="midpoint", return_trajectory=True, **step_kw, **k)  # noqa: E731
    sched0 = run()
    rule0 = run(rescale=0.7, norm_limit=1.0)
    before = eng.graph_replays()
    apg = dict(eta=0.5, momentum=0.5, norm_threshold=40.0)
    got = run(apg=apg)
    # the conditional key has been used by the calls above, the projected key is new: its first use runs eagerly, every later one replays
    assert eng.graph_replays() - before == (G_ - 1) + C_
    assert eng.last_nfe() == 8 and eng.last_eval_rows() == 2 * G_ + C_
    want = G.sample_cfg_project(model, z, tgrid, table, "midpoint", apg=apg, cap_feats=cap, cap_mask=cmask, **step_kw)
    for i in range(len(tgrid)):
        assert torch.equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    # other parameters: no new key - every evaluation replays - and another result, the host loop's
    before = eng.graph_replays()
    apg2 = dict(eta=0.0, momentum=-0.25, norm_threshold=25.0)
    got2 = run(apg=apg2)
    assert eng.graph_replays() - before == G_ + C_
    want2 = G.sample_cfg_project(model, z, tgrid, table, "midpoint", apg=apg2, cap_feats=cap, cap_mask=cmask, **step_kw)
    assert torch.equal(got2, want2) and not torch.equal(got2[-1], got[-1])
    # the other form is a key of its own
    before = eng.graph_replays()
    gz = run(zero_star=True)
    assert eng.graph_replays() - before == (G_ - 1) + C_
    assert torch.equal(gz, G.sample_cfg_project(model, z, tgrid, table, "midpoint", zero_star=True, cap_feats=cap, cap_mask=cmask, **step_kw))
    # the schedule call and the rule call replay their keys of before and give the trajectories they gave
    before = eng.graph_replays()
    assert torch.equal(run(), sched0) and torch.equal(run(rescale=0.7, norm_limit=1.0), rule0)
    assert eng.graph_replays() - before == 2 * (G_ + C_)


# ---- front end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["imagenet", "flag"])
def test_other_families_run_the_same_call_through_the_transport_front_end(golden_dir, family):
    model, z, kw = _model(golden_dir, family)
    z = z.to("cuda", torch.bfloat16)
    assert z.shape[0] == 2 and z.shape[1] > 3  # guidance on 3 of more channels
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), **kw)  # the flags a plain forward reads
    o = ODE(5, "midpoint", 4)
    table = torch.tensor([1.0, 1.0, 2.0, 1.0, 4.0, 3.0, 1.0, 1.0])
    off = o.sample(z, model.forward_with_cfg, cfg_table=table, **kw)
    for extra, nfe, rows in ((dict(cfg_apg=dict(eta=0.0, momentum=0.5, norm_threshold=30.0)), 8, 2 * 3 + 5),
                             (dict(cfg_zero_star=True), 8, 2 * 3 + 5), (dict(cfg_zero_star=True, cfg_zero_init=1), 6, 2 * 3 + 3)):
        o.use_engine = True
        got = o.sample(z, model.forward_with_cfg, cfg_table=table, **extra, **kw)
        assert model._engine.last_nfe() == nfe and model._engine.last_eval_rows() == rows, (family, extra)
        o.use_engine = False
        want = o.sample(z, model.forward_with_cfg, cfg_table=table, **extra, **kw)
        assert got.shape == (5,) + tuple(z.shape) and bool(torch.isfinite(want.float()).all())
        for i in range(5):
            assert torch.equal(got[i], want[i]), (family, extra, i)
        assert not torch.equal(got[-1], off[-1])
    # without a table: cfg_scale at every stage, on the engine and on the host
    o.use_engine = True
    const = o.sample(z, model.forward_with_cfg, cfg_zero_star=True, **kw)
    assert model._engine.last_nfe() == 8 and model._engine.last_eval_rows() == 16
    o.use_engine = False
    assert torch.equal(const, o.sample(z, model.forward_with_cfg, cfg_zero_star=True, **kw))


def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    n = 2 * 4 * 16 * 16
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    lim = model.engine_limits  # room for a batch of 3: the odd batch must reach its own refusal
    model.engine_limits = EngineLimits(max(lim.max_batch, 6), lim.max_tokens, lim.max_text)
    t = torch.full((2,), 0.5, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0)  # engine, weights, a prompt of 2 rows
    eng, L = model._engine, lib()
    out = torch.full((8 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    grid = (C.c_float * 3)(0.0, 0.5, 1.0)
    good = (C.c_float * 2)(4.0, 1.0)
    nan = float("nan")

    def traj(*, form=APG, eta=0.5, beta=0.5, r=1.0, K=0, batch=2, tab=good, ng=3, method=0):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        return L.lt_sample_ode_cfg_project(eng.handle, P(z), P(out), P(out[4 * n:]), grid, ng, method, tab, form, eta, beta, r, K, 1, C.byref(a), stream())

    def one(*, form=APG, eta=0.5, beta=0.5, r=1.0, keep=0, batch=2, scale=4.0):
        a = eng._step_args(z, scale, 1.0, 1.0, None, False)
        a.batch = batch
        return L.lt_forward_cfg_project(eng.handle, P(z), P(t), P(out), form, eta, beta, r, keep, C.byref(a), stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    for call, who in ((traj, "lt_sample_ode_cfg_project:"), (one, "lt_forward_cfg_project:")):
        refused(call(form=0), who, "form")
        refused(call(form=3), who, "form")
        refused(call(eta=nan), who, "eta")
        refused(call(eta=INF), who, "eta")
        refused(call(beta=1.0), who, "momentum")
        refused(call(beta=-1.5), who, "momentum")
        refused(call(beta=nan), who, "momentum")
        refused(call(r=0.0), who, "norm_threshold")
        refused(call(r=-2.0), who, "norm_threshold")
        refused(call(r=nan), who, "norm_threshold")
        refused(call(batch=3), who, "even batch")
    refused(traj(tab=(C.c_float * 2)(4.0, nan)), "lt_sample_ode_cfg_project:", "not finite")
    refused(traj(ng=1), "lt_sample_ode_cfg_project:", "2 grid points")
    refused(traj(method=7), "lt_sample_ode_cfg_project:", "unknown method")
    refused(traj(tab=None), "lt_sample_ode_cfg_project:", "null argument")
    refused(traj(form=ZERO, K=2), "lt_sample_ode_cfg_project:", "zero_init")
    refused(traj(form=ZERO, K=-1), "lt_sample_ode_cfg_project:", "zero_init")
    refused(traj(K=1), "lt_sample_ode_cfg_project:", "zero_init", "CFG-Zero*")
    refused(one(scale=nan), "lt_forward_cfg_project:", "not finite")
    refused(one(keep=2), "lt_forward_cfg_project:", "keep_momentum")
    refused(one(form=ZERO, keep=1), "lt_forward_cfg_project:", "keep_momentum")
    eng.prepare_prompt_regional(cap, cmask, cap[:1].contiguous(), cmask[:1].contiguous(), 1, 1)
    refused(traj(), "lt_sample_ode_cfg_project:", "regional prompt")
    refused(one(), "lt_forward_cfg_project:", "regional prompt")
    eng.prepare_prompt(cap, cmask)
    refused(one(keep=1), "lt_forward_cfg_project:", "no stored momentum")
    # the Python layers refuse the same parameters, the companions and a packed batch, before any engine call
    tg, tb = [0.0, 0.5, 1.0], torch.tensor([4.0, 4.0])
    apg = dict(eta=0.5)
    sched = lambda **k: model.sample_ode_cfg_schedule(z, tg, tb, cap, cmask, method=k.pop("method", "euler"), **k)  # noqa: E731
    for words, k in (("exclusive", dict(apg=apg, zero_star=True)), ("eta", dict(apg=dict(eta=nan))), ("momentum", dict(apg=dict(momentum=1.0))),
                     ("norm_threshold", dict(apg=dict(norm_threshold=0.0))), ("not \\['beta'\\]", dict(apg=dict(beta=0.5))),
                     ("zero_init", dict(zero_init=1)), ("zero_init", dict(zero_star=True, zero_init=2)),
                     ("rescale / norm_limit", dict(apg=apg, rescale=0.5)), ("rescale / norm_limit", dict(zero_star=True, norm_limit=1.0)),
                     ("reuse", dict(apg=apg, reuse=[0, 1])), ("slg", dict(zero_star=True, slg=[0.5, 0.5], slg_layers=[0])),
                     ("pag", dict(apg=apg, pag=[0.5, 0.5], pag_layers=[0])), ("fixed-grid", dict(apg=apg, method="abm2")),
                     ("fixed-grid", dict(zero_star=True, method="ab3"))):
        with pytest.raises(_lib.LuminaLibError, match=words):
            sched(**k)
    with pytest.raises(_lib.LuminaLibError, match="packed"):
        model.sample_ode_cfg_schedule([z[0], z[1]], tg, tb, cap, cmask, method="euler", apg=apg)
    with pytest.raises(_lib.LuminaLibError, match="packed"):
        model.forward_with_cfg_project([z[0], z[1]], t, cap, cmask, 4.0, zero_star=True)
    with pytest.raises(_lib.LuminaLibError, match="exclusive"):
        model.forward_with_cfg_project(z, t, cap, cmask, 4.0, apg=apg, zero_star=True)
    o = ODE(3, "euler")
    zc = z.clone()
    for words, k in (("teacache", dict(cfg_apg=apg, teacache=0.1)), ("mask", dict(cfg_zero_star=True, mask=torch.ones_like(z), x1=z, noise=z)),
                     ("exclusive", dict(cfg_apg=apg, cfg_zero_star=True)), ("adaptive|fixed-grid", dict(cfg_apg=apg, _method="dopri5"))):
        oo = ODE(3, k.pop("_method")) if "_method" in k else o
        with pytest.raises((ValueError, _lib.LuminaLibError), match=words):
            oo.sample(z, model.forward_with_cfg, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **k)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and torch.equal(z, zc)
    # ... and the same arguments untouched are served; forward_with_cfg goes on as before
    assert traj() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:3 * n].float()).all()) and eng.last_nfe() == 2 and eng.last_eval_rows() == 3
    assert one() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:n].float()).all())
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0), ref)


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_sample_driver_with_a_projected_form_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_project_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_project_test"] = ctor
    (tmp_path / "prompts.txt").write_text("a red cube\n")
    gen = torch.Generator().manual_seed(3)
    table = {c: torch.randn(16, cfg.cap_feat_dim, generator=gen) for c in ("a red cube", "")}

    def encode(caps):
        feats = torch.stack([table[c] for c in caps]).to("cuda", torch.bfloat16)
        mask = torch.ones(len(caps), 16, dtype=torch.int64, device="cuda")
        mask[-1, 8:] = 0
        return feats, mask

    decoded = []

    def decode(lat):
        decoded.append(lat.clone())
        return torch.sigmoid(lat[:, :3].float())

    argv = ["--ckpt", str(ck), "--caption_path", str(tmp_path / "prompts.txt"), "--resolution", "256:128x128", "--num_sampling_steps", "5",
            "--sampling-method", "midpoint", "--time_shifting_factor", "4", "--seed", "11"]
    runs = {}
    try:
        for name, extra in (("default", []), ("apg", ["--apg_eta", "0.25", "--apg_momentum", "-0.5", "--apg_norm_threshold", "20"]),
                            ("interval", ["--apg_eta", "0.25", "--cfg_interval", "0.1", "0.8"]),
                            ("zero", ["--cfg_zero_star", "--cfg_zero_init", "1"])):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            runs[name] = (built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
    finally:
        del models.__dict__["NextDiT_tiny_project_test"]
    fn = Sampler(create_transport()).sample_ode(sampling_method="midpoint", num_steps=5, time_shifting_factor=4.0)
    tgrid = fn.__self__.t
    itab = G.cfg_table(tgrid, "midpoint", 4.0, interval=(0.1, 0.8))
    Gi, Ci = int((itab != 1).sum()), int((itab == 1).sum())
    # every evaluation of a run lies in ONE whole-trajectory call
    assert runs == {"default": (8, 16), "apg": (8, 16), "interval": (8, 2 * Gi + Ci), "zero": (6, 12)}
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    feats, mask = encode(["a red cube", ""])
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    # the default invocation is the call it was
    want = fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1]
    assert torch.equal(decoded[0], want / 0.13025)
    full = G.cfg_table(tgrid, "midpoint", 4.0)
    apg = dict(eta=0.25, momentum=-0.5, norm_threshold=20.0)
    want = model.sample_ode_cfg_schedule(z, tgrid, full, feats, mask, method="midpoint", apg=apg, **kw)[:1]
    assert bool(torch.isfinite(decoded[1].float()).all()) and torch.equal(decoded[1], want / 0.13025) and not torch.equal(decoded[1], decoded[0])
    want = model.sample_ode_cfg_schedule(z, tgrid, itab, feats, mask, method="midpoint", apg=dict(eta=0.25), **kw)[:1]
    assert torch.equal(decoded[2], want / 0.13025) and not torch.equal(decoded[2], decoded[1])
    want = model.sample_ode_cfg_schedule(z, tgrid, full, feats, mask, method="midpoint", zero_star=True, zero_init=1, **kw)[:1]
    assert torch.equal(decoded[3], want / 0.13025) and not torch.equal(decoded[3], decoded[0])
