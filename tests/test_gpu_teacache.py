"""GPU: step caching - lt_op_cache_* / lt_forward_cached / lt_sample_ode_cached.

* kernels word for word: store and apply against the bf16 chain on operands that sit on its rounding edges; the indicator's sums exact on
  integer operands and within the derived float64 bound on random ones, in both layouts, one shape past a single grid pass;
* a run evaluation (probe, then run) is the plain forward bit for bit, four families, both state dtypes, below and above the graph threshold;
* a reuse evaluation: the token stream is bf16(x0 + r) word for word on the engine's own buffers, and on a model whose gates are zero (r = 0)
  the reuse at another time is that model's plain forward there - the modulation is this evaluation's, the tail is the plain tail;
* the engine's trajectory equals the host loop ``transport.cache.sample_teacache`` state for state, decisions and indicator included;
* the ends (threshold 0, a huge threshold), the graph path, the other families, refusals by name, the ``sample.py`` driver."""
import ctypes as C

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import cache as TC
from lumina_t2x_amd.transport.mini import ODE

import exact_cache as X
import exact_rows as R
import exact_slg as XS
from gpu_util import P, lib, stream
from test_gpu_slg import FAMILIES, STEP_KW, _build, _deep

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
GUARD = 64
HUGE = 1e30
_CACHE = {}


def _guarded(t, fill=1.5):
    buf = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype, device="cuda")
    buf[GUARD:-GUARD] = t.reshape(-1).cuda()
    return buf


def _guards_ok(buf, fill=1.5):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


# ---- 1. kernels ----------------------------------------------------------------------------------------------------------------------
# rows x d; the last has 131 840 chunks of 8 words, past the 512 * 256 = 131 072 chunks of one grid pass
SHAPES = [(1, 64), (3, 72), (130, 256), (1030, 1024)]


@pytest.mark.parametrize("rows,d", SHAPES, ids=[f"{r}x{d}" for r, d in SHAPES])
def test_residual_store_and_apply_word_for_word(rows, d):
    L = lib()
    n = rows * d
    assert rows * d // 8 > 512 * 256 or rows < 1030
    xl, x0 = X.edge_operands(n, 11 + rows)
    a, b = _guarded(xl), _guarded(x0)
    r = torch.full((n + 2 * GUARD,), 1.5, dtype=torch.bfloat16, device="cuda")
    assert L.lt_op_cache_residual_store(P(a[GUARD:]), P(b[GUARD:]), P(r[GUARD:]), n, stream()) == 0, L.lt_last_error()
    torch.cuda.synchronize()
    want = X.ref_store(xl, x0)
    assert torch.equal(X.bits(r[GUARD:-GUARD].cpu()), X.bits(want)), int((X.bits(r[GUARD:-GUARD].cpu()) != X.bits(want)).sum())
    assert _guards_ok(r) and torch.equal(X.bits(a[GUARD:-GUARD].cpu()), X.bits(xl)) and torch.equal(X.bits(b[GUARD:-GUARD].cpu()), X.bits(x0))
    # apply: x <- bf16(x + r) on the same edge operands (the rows' h is then not finite everywhere: checked on a plain draw below)
    B, N = (1, rows) if rows % 2 else (2, rows // 2)
    mod, ld = R.draw_mod(B, 2 * d + 24, 5 + rows), 2 * d + 24
    ns, nsh = mod[:, 8:8 + d], mod[:, 8 + d:8 + 2 * d]
    dev_mod = mod.clone()
    dev_mod[:, 8:8 + d] = (1.0 + ns.float()).to(torch.bfloat16)
    dev_mod = dev_mod.cuda()
    sub = lambda i: C.c_void_p(dev_mod.data_ptr() + 2 * (8 + i * d))  # noqa: E731
    h = torch.full((n + 2 * GUARD,), 1.5, dtype=torch.bfloat16, device="cuda")
    x = _guarded(xl)
    rr = _guarded(x0)
    assert L.lt_op_cache_residual_apply(P(x[GUARD:]), P(rr[GUARD:]), sub(0), sub(1), ld, P(h[GUARD:]), B, N, d, stream()) == 0, L.lt_last_error()
    torch.cuda.synchronize()
    want = X.ref_apply_x(xl, x0)
    assert torch.equal(X.bits(x[GUARD:-GUARD].cpu()), X.bits(want)), int((X.bits(x[GUARD:-GUARD].cpu()) != X.bits(want)).sum())
    assert _guards_ok(x) and _guards_ok(h) and _guards_ok(rr)
    # a plain draw: x' word for word, h against the float64 chain of gated_residual_norm's next_mode 2 (tests/exact_rows.py), with and without shift
    xa, ra = R.draw_rows(B * N, d, d + 1, std=1.0, mean_rows=True), R.draw_rows(B * N, d, d + 2, std=2.0)
    for shift in (True, False):
        x, rr = _guarded(xa), _guarded(ra)
        h = torch.full((n + 2 * GUARD,), 1.5, dtype=torch.bfloat16, device="cuda")
        rc = L.lt_op_cache_residual_apply(P(x[GUARD:]), P(rr[GUARD:]), sub(0), sub(1) if shift else None, ld, P(h[GUARD:]), B, N, d, stream())
        assert rc == 0, L.lt_last_error()
        torch.cuda.synchronize()
        xd = x[GUARD:-GUARD].view(B * N, d)
        assert torch.equal(X.bits(xd.cpu()), X.bits(X.ref_apply_x(xa, ra)))
        ch = R.ref_gated_h(xd, None, dev_mod.cpu()[:, 8:8 + d], nsh if shift else None, B, N, 1e-6, 1e-6, 2, 1)  # (the prepared bf16(1 + scale))
        R.assert_row_words(h[GUARD:-GUARD].view(B * N, d), ch, f"cache apply {rows}x{d} shift {shift}", N=N)
        assert _guards_ok(x) and _guards_ok(h)


def _indicator(h, hp, pair, rows, d):
    L = lib()
    a, b = _guarded(h), _guarded(hp)
    if pair:
        for t in (a, b):
            assert L.lt_op_pair_layout(P(t[GUARD:]), rows, d, 1, stream()) == 0, L.lt_last_error()
    ws = torch.zeros(L.lt_op_cache_ws_bytes() // 8 + 2 * GUARD, dtype=torch.float64, device="cuda")
    sums = torch.full((2 + 2 * GUARD,), 1.5, dtype=torch.float64, device="cuda")
    kept = a.clone()
    assert L.lt_op_cache_indicator(P(a[GUARD:]), P(b[GUARD:]), rows * d, P(ws[GUARD:]), P(sums[GUARD:]), stream()) == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert torch.equal(X.bits(b[GUARD:-GUARD]), X.bits(a[GUARD:-GUARD])) and torch.equal(X.bits(a), X.bits(kept))  # h_prev == h bit for bit
    assert _guards_ok(b) and _guards_ok(sums) and bool((ws[:GUARD] == 0).all()) and bool((ws[-GUARD:] == 0).all())
    return float(sums[GUARD]), float(sums[GUARD + 1])


@pytest.mark.parametrize("pair", [0, 1], ids=["rowmajor", "pair"])
@pytest.mark.parametrize("rows,d", SHAPES, ids=[f"{r}x{d}" for r, d in SHAPES])
def test_indicator_sums_and_h_prev(rows, d, pair):
    if pair and (rows % 2 or d % 32):
        pair = 0  # (the pair layout needs an even row count and d % 32 == 0: such a shape is checked row-major only)
    n = rows * d
    ia, ib = X.integer_operands(n, 3 + rows)
    assert _indicator(ia, ib, pair, rows, d) == X.ref_sums(ia, ib)  # exact integers, whatever the order
    g = torch.Generator().manual_seed(7 + rows)
    ha, hb = torch.randn(n, generator=g).to(torch.bfloat16), torch.randn(n, generator=g).mul(2).to(torch.bfloat16)
    s1, s0 = _indicator(ha, hb, pair, rows, d)
    w1, w0 = X.ref_sums(ha, hb)
    print(f"TEACACHE indicator {rows}x{d} pair {pair}: S1 rel err {abs(s1 - w1) / w1:.3e} S0 rel err {abs(s0 - w0) / w0:.3e} bound {X.sum_bound(n):.3e}")
    assert abs(s1 - w1) <= X.sum_bound(n) * w1 and abs(s0 - w0) <= X.sum_bound(n) * w0
    # identical operands: S1 is an exact zero; a zero h_prev: S0 is
    assert _indicator(ha, ha.clone(), pair, rows, d)[0] == 0.0
    assert _indicator(ha, torch.zeros_like(ha), pair, rows, d)[1] == 0.0


def test_kernel_refusals():
    L = lib()
    t = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(L.lt_op_cache_ws_bytes() // 8, dtype=torch.float64, device="cuda")
    s = torch.zeros(2, dtype=torch.float64, device="cuda")
    for call, word in ((lambda: L.lt_op_cache_indicator(P(t), P(t), 60, P(ws), P(s), stream()), "16-byte"),
                       (lambda: L.lt_op_cache_indicator(P(t), None, 64, P(ws), P(s), stream()), "null"),
                       (lambda: L.lt_op_cache_residual_store(P(t), P(t), P(t), 0, stream()), "16-byte"),
                       (lambda: L.lt_op_cache_residual_store(P(t), None, P(t), 64, stream()), "null"),
                       (lambda: L.lt_op_cache_residual_apply(P(t), P(t), None, None, 64, P(t), 1, 1, 64, stream()), "null")):
        rc = call()
        assert rc != 0 and word in L.lt_last_error().decode(), L.lt_last_error()


# ---- engine ----------------------------------------------------------------------------------------------------------------------------
def _family(golden_dir, family):
    """(model, engine evaluator args for guided and plain evaluations) of the family's four-block model"""
    if family not in _CACHE:
        cfg, sd, cond = _deep(golden_dir, family)
        _CACHE[family] = (_build(family, cfg, sd), cond, cfg, sd)
    return _CACHE[family]


def _kw(model, cond, family, guided=True):
    kw = dict(zip(model._cond_names, cond))
    if guided:
        kw["cfg_scale"] = 4.0
        if family in ("next", "flag"):
            kw.update(STEP_KW)
    return kw


def _read(eng, which, n):
    out = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    _lib.check(eng.lib.lt_debug_cache_read(eng.handle, which, P(out), n, stream()), "lt_debug_cache_read")
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_probe_then_run_is_the_plain_forward_bit_for_bit(golden_dir, family, dtype):
    model, cond, _, _ = _family(golden_dir, family)
    g = torch.Generator().manual_seed(21)
    t = torch.tensor([0.25, 0.75], device="cuda")
    for H in (16, 48):  # 128 rows: plain launches; 1152 rows: through the graph cache
        z = torch.randn(2, 4, H, H, generator=g).to("cuda", dtype)
        for use_cfg in (True, False):
            kw = _kw(model, cond, family)
            if use_cfg:
                model._mirror_attention_flags(kw)
            else:
                kw.pop("cfg_scale")
                for k in STEP_KW:
                    kw.pop(k, None)
            eng, args = model._engine_sampler_args(z, use_cfg, kw)
            want = eng.forward(z, t, use_cfg=use_cfg, **args)
            for rep in range(3):  # eager, capture + replay, replay
                s1, s0 = eng.forward_cached(z, t, "probe", use_cfg=use_cfg, **args)
                got = eng.forward_cached(z, t, "run", use_cfg=use_cfg, **args)
                assert torch.equal(got, want), (family, dtype, H, use_cfg, rep, int((got != want).sum()))
                assert rep == 0 or s1 == 0.0  # the same h twice
            assert torch.equal(eng.forward(z, t, use_cfg=use_cfg, **args), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_reuse_is_its_definition(golden_dir, dtype):
    model, cond, cfg, sd = _family(golden_dir, "next")
    g = torch.Generator().manual_seed(23)
    ta, tb = torch.tensor([0.25, 0.25], device="cuda"), torch.tensor([0.625, 0.625], device="cuda")
    for H in (16, 48):
        za, zb = (torch.randn(2, 4, H, H, generator=g).to("cuda", dtype) for _ in range(2))
        kw = _kw(model, cond, "next")
        model._mirror_attention_flags(kw)
        eng, args = model._engine_sampler_args(za, True, kw)
        n = 2 * (H // 2) ** 2 * cfg.dim
        for rep in range(3):
            eng.forward_cached(za, ta, "probe", use_cfg=True, **args)
            x0a = _read(eng, 1, n)
            eng.forward_cached(za, ta, "run", use_cfg=True, **args)
            xla, r = _read(eng, 3, n), _read(eng, 2, n)
            assert torch.equal(X.bits(r), X.bits(X.ref_store(xla, x0a))), (H, rep)
            assert bool((r != 0).any())
            eng.forward_cached(zb, tb, "probe", use_cfg=True, **args)
            x0b = _read(eng, 1, n)
            assert not torch.equal(x0a, x0b)
            out = eng.forward_cached(zb, tb, "reuse", use_cfg=True, **args)
            x = _read(eng, 3, n)
            assert torch.equal(X.bits(x), X.bits(X.ref_apply_x(x0b, r))), (H, rep, int((X.bits(x) != X.bits(X.ref_apply_x(x0b, r))).sum()))
            assert torch.equal(X.bits(_read(eng, 2, n)), X.bits(r))  # a reuse leaves the residual as it is
            # h: the final layer's LayerNorm + modulate of x with THIS evaluation's modulation - the plain forward of zb at tb prepared the same
            # modulation, and a model whose blocks add nothing shows it (below); here: the output is finite and not the run's
            assert bool(torch.isfinite(out.float()).all()) and not torch.equal(out, eng.forward(zb, tb, use_cfg=True, **args))
    # blocks that add nothing (every gate zero): x_L == x_0, r == 0, and the reuse at (zb, tb) after a run at (za, ta) IS the plain forward at
    # (zb, tb) - final norm, this evaluation's modulation, final GEMM, closing kernel
    ident = _build("next", cfg, XS.zero_gates(sd, cfg.family, tuple(range(cfg.n_layers)), cfg.dim))
    for H in (16, 48):
        za, zb = (torch.randn(2, 4, H, H, generator=g).to("cuda", dtype) for _ in range(2))
        for use_cfg in (True, False):
            kw = _kw(ident, cond, "next")
            if use_cfg:
                ident._mirror_attention_flags(kw)
            else:
                kw.pop("cfg_scale")
                for k in STEP_KW:
                    kw.pop(k, None)
            eng, args = ident._engine_sampler_args(za, use_cfg, kw)
            want = eng.forward(zb, tb, use_cfg=use_cfg, **args)
            for rep in range(3):
                eng.forward_cached(za, ta, "probe", use_cfg=use_cfg, **args)
                eng.forward_cached(za, ta, "run", use_cfg=use_cfg, **args)
                assert not bool(_read(eng, 2, 2 * (H // 2) ** 2 * cfg.dim).any())
                eng.forward_cached(zb, tb, "probe", use_cfg=use_cfg, **args)
                got = eng.forward_cached(zb, tb, "reuse", use_cfg=use_cfg, **args)
                assert torch.equal(got, want), (H, use_cfg, rep, int((got != want).sum()))


# ---- 4. trajectory ---------------------------------------------------------------------------------------------------------------------
# threshold and the hit pattern it gives on ODE(n, method, 4)'s grid (1 = the stack ran), picked on the engine's recorded rel values of the
# four-block nextdit golden at 2 x 4 x 16 x 16 (printed by the test as TEACACHE rel ...): see PICKED below
PICKED = {
    # method: (grid points, threshold, pattern); recorded rel at threshold 0 (bf16; fp32 agrees to three digits):
    #   euler    .170 .198 .193 .209 .233 .234           one rel stays below 0.27, two in a row pass it
    #   midpoint .145 .169 .160 .158 .200 .195 .205 .210  likewise
    #   rk4      .183 .295 .527 .384 .253 .342 .465 .305 .291 .508; a reuse changes what follows, so the rk4 threshold was picked on the
    #            accumulator recorded AT 0.45: .183 .360 .520 .058 .307 .499 .398 .621 .323 .485 - no value within 0.03 of it
    "euler": (9, 0.27, (1, 0, 1, 0, 1, 0, 1, 1)),
    "midpoint": (6, 0.27, (1, 0, 1, 0, 1, 0, 1, 0, 1, 1)),
    "rk4": (4, 0.45, (1, 0, 0, 1, 0, 0, 1, 0, 1, 0, 1, 1)),
}


def _pattern_ok(p):
    runs_after_first = sum(p[1:])
    reuses = len(p) - sum(p)
    reuse_then_run = any(a == 0 and b == 1 for a, b in zip(p, p[1:]))
    return reuses >= 2 and runs_after_first >= 2 and reuse_then_run


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, (cap, cmask), cfg, _ = _family(golden_dir, "next")
    points, thr, pattern = PICKED[method]
    tgrid = ODE(points, method, 4).t
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(6)).to("cuda", dtype).repeat(2, 1, 1, 1)
    ncalls = (points - 1) * STAGES[method]
    got = model.sample_ode_teacache(z, tgrid, cap, cmask, 4.0, method=method, threshold=thr, return_trajectory=True, **STEP_KW)
    eng_stats = dict(model.last_cache_stats)
    want = model.sample_ode_teacache(z, tgrid, cap, cmask, 4.0, method=method, threshold=thr, return_trajectory=True, host_loop=True, **STEP_KW)
    host_stats = dict(model.last_cache_stats)
    n = 2 * 64 * cfg.dim
    print(f"TEACACHE rel {method} {dtype}: " + " ".join(f"{v:.6f}" for v in host_stats["stats"][:, 0].tolist()))
    print(f"TEACACHE acc {method} {dtype}: " + " ".join(f"{v:.6f}" for v in host_stats["stats"][:, 1].tolist()))
    ran = [int(v) for v in host_stats["stats"][:, 2].tolist()]
    assert len(ran) == ncalls and ran == list(pattern) and _pattern_ok(ran), ran
    # the proviso, on the host loop's values: no accumulator within the bound of the threshold
    thr32 = TC.check_cache_args(thr)[0]
    for j, acc in enumerate(host_stats["stats"][:, 1].tolist()):
        if 0 < j < ncalls - 1:
            assert abs(acc - thr32) > X.rel_bound(n) * ncalls * max(abs(acc), thr32), (j, acc, thr32)
    for j in range(ncalls):
        a, b = float(eng_stats["stats"][j, 0]), float(host_stats["stats"][j, 0])
        assert abs(a - b) <= X.rel_bound(n) * abs(b), (j, a, b)
    assert [int(v) for v in eng_stats["stats"][:, 2].tolist()] == ran
    hits = ncalls - sum(ran)
    assert eng_stats["hits"] == host_stats["hits"] == hits and eng_stats["nfe"] == ncalls and eng_stats["rows"] == 2 * sum(ran)
    assert got.shape == want.shape == (points,) + tuple(z.shape) and bool(torch.isfinite(want.float()).all())
    for i in range(points):
        assert torch.equal(got[i], want[i]), (method, dtype, i, int((got[i] != want[i]).sum()))
    # ... and it is not the trajectory without the cache
    plain = ODE(points, method, 4).sample(z, model.forward_with_cfg, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **STEP_KW)
    assert not torch.equal(plain[-1], got[-1])


# ---- 5. ends ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_threshold_zero_is_the_plain_trajectory_and_a_huge_one_runs_the_ends_alone(golden_dir, method, dtype):
    model, (cap, cmask), _, _ = _family(golden_dir, "next")
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(8)).to("cuda", dtype).repeat(2, 1, 1, 1)
    o = ODE(5, method, 4)
    ncalls = 4 * STAGES[method]
    plain = o.sample(z, model.forward_with_cfg, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **STEP_KW)
    got = model.sample_ode_teacache(z, o.t, cap, cmask, 4.0, method=method, threshold=0.0, return_trajectory=True, **STEP_KW)
    st = model.last_cache_stats
    assert torch.equal(got, plain) and st["hits"] == 0 and st["rows"] == ncalls * 2 and st["nfe"] == ncalls
    via = o.sample(z, model.forward_with_cfg, teacache=0.0, cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **STEP_KW)
    assert torch.equal(via, plain)
    if method == "euler":
        # a single interval: the one evaluation is first and last
        one = ODE(2, "euler", 4)
        got = model.sample_ode_teacache(z, one.t, cap, cmask, 4.0, method="euler", threshold=HUGE, return_trajectory=True, **STEP_KW)
        assert model.last_cache_stats["hits"] == 0 and torch.equal(got, one.sample(z, model.forward_with_cfg, cap_feats=cap, cap_mask=cmask,
                                                                                  cfg_scale=4.0, **STEP_KW))
        six = ODE(7, "euler", 4)
        model.sample_ode_teacache(z, six.t, cap, cmask, 4.0, method="euler", threshold=HUGE, **STEP_KW)
        st = model.last_cache_stats
        assert st["hits"] == 4 and st["rows"] == 2 * 2 and st["nfe"] == 6
        assert [int(v) for v in st["stats"][:, 2].tolist()] == [1, 0, 0, 0, 0, 1]


# ---- 6. graph path -----------------------------------------------------------------------------------------------------------------------
def test_graph_path_replays_three_keys_whatever_the_threshold(golden_dir):
    cfg, sd, (cap, cmask) = _deep(golden_dir, "next")
    model = _build("next", cfg, sd)  # a fresh engine: its graph cache is this test's
    z = torch.randn(1, 4, 48, 48, generator=torch.Generator().manual_seed(9)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)  # 1152 rows
    t = torch.tensor([0.5, 0.5], device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    o = ODE(7, "euler", 4)
    outs = {}
    model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    # 6 evaluations = 12 segments either way (6 heads + 6 stacks; 6 heads + 2 stacks + 4 reuses).  The first use of a key runs as plain
    # launches, every later one replays: the threshold is no part of a key, and a trajectory has three
    for thr, first_uses in ((0.0, 2), (HUGE, 1), (0.0, 0), (HUGE, 0)):
        before = model._engine.graph_replays()
        outs.setdefault(thr, []).append(model.sample_ode_teacache(z, o.t, cap, cmask, 4.0, threshold=thr, return_trajectory=True, **STEP_KW))
        assert model._engine.graph_replays() - before == 12 - first_uses, (thr, model._engine.graph_replays() - before)
    assert torch.equal(outs[0.0][0], outs[0.0][1]) and torch.equal(outs[HUGE][0], outs[HUGE][1])
    model._engine.set_option("graph", 0)
    for thr in (0.0, HUGE):
        eager = model.sample_ode_teacache(z, o.t, cap, cmask, 4.0, threshold=thr, return_trajectory=True, **STEP_KW)
        assert torch.equal(eager, outs[thr][0]), thr
    model._engine.set_option("graph", None)
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW), ref)


# ---- 7. other families -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["imagenet", "flag", "moe"])
def test_other_families_engine_equals_host_loop_through_the_front_end(golden_dir, family):
    model, cond, _, _ = _family(golden_dir, family)
    kw = _kw(model, cond, family)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(10)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    o = ODE(7, "midpoint", 4)
    for thr in (HUGE, 0.0):
        got = o.sample(z, model.forward_with_cfg, teacache=thr, **kw)
        st = dict(model.last_cache_stats)
        cond_kw = {k: kw[k] for k in model._cond_names}
        step_kw = {k: v for k, v in kw.items() if k not in model._cond_names}
        want = model.sample_ode_teacache(z, o.t, *[cond_kw[k] for k in model._cond_names], threshold=thr, method="midpoint", return_trajectory=True,
                                         host_loop=True, **step_kw)
        assert model.last_cache_stats["hits"] == st["hits"] == (10 if thr else 0) and st["nfe"] == 12
        for i in range(7):
            assert torch.equal(got[i], want[i]), (family, thr, i, int((got[i] != want[i]).sum()))


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_outputs_and_state_untouched(golden_dir):
    model, (cap, cmask), cfg, _ = _family(golden_dir, "next")
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(12)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    t = torch.tensor([0.5, 0.5], device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    o = ODE(5, "euler", 4)
    base = dict(cap_feats=cap, cap_mask=cmask, cfg_scale=4.0, **STEP_KW)
    four = torch.full((4,), 4.0)

    def check(exc_type, word, fn):
        with pytest.raises(exc_type, match=word):
            fn()
        assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW), ref), word  # a following plain call gives its old result

    check(ValueError, "cfg_table", lambda: o.sample(z, model.forward_with_cfg, teacache=0.1, cfg_table=four, **base))
    check(ValueError, "cfg_rescale", lambda: o.sample(z, model.forward_with_cfg, teacache=0.1, cfg_rescale=0.5, **base))
    check(ValueError, "cfg_norm_limit", lambda: o.sample(z, model.forward_with_cfg, teacache=0.1, cfg_norm_limit=2.0, **base))
    check(ValueError, "cfg_reuse", lambda: o.sample(z, model.forward_with_cfg, teacache=0.1, cfg_reuse=[0, 1, 0, 1], **base))
    check(ValueError, "skip-layer", lambda: o.sample(z, model.forward_with_cfg, teacache=0.1, slg_table=four, slg_layers=[1], **base))
    check(ValueError, "mask", lambda: o.sample(z, model.forward_with_cfg, teacache=0.1, mask=torch.ones_like(z), x1=z, noise=z, **base))
    check(ValueError, "packed batch", lambda: o.sample([z[0], z[1]], model.forward_with_cfg, teacache=0.1, **base))
    check(ValueError, "multistep", lambda: ODE(5, "abm2", 4).sample(z, model.forward_with_cfg, teacache=0.1, **base))
    check(ValueError, "adaptive", lambda: ODE(5, "dopri5", 4).sample(z, model.forward_with_cfg, teacache=0.1, **base))
    check(_lib.LuminaLibError, "packed batch", lambda: model.sample_ode_teacache([z[0], z[1]], o.t, cap, cmask, 4.0, threshold=0.1, **STEP_KW))
    check(_lib.LuminaLibError, ">= 0", lambda: model.sample_ode_teacache(z, o.t, cap, cmask, 4.0, threshold=-1.0, **STEP_KW))
    eng = model._engine
    args = dict(cfg_scale=4.0, **STEP_KW)
    # the C entry itself: threshold, coefficients, method, capture-free refusals with the outputs untouched
    a = eng._step_args(z, 4.0, 1.0, 1.0, 16, True)
    out = torch.full((5,) + tuple(z.shape), float("nan"), dtype=z.dtype, device="cuda")
    grid = (C.c_float * 5)(*[float(v) for v in o.t])
    ident = (C.c_double * 5)(0, 0, 0, 1, 0)

    def centry(method=0, thr=0.1, coef=ident):
        return eng.lib.lt_sample_ode_cached(eng.handle, P(z), P(out), None, grid, 5, method, 1, 1, C.byref(a), thr, coef, None, stream())

    for kwargs, word in ((dict(method=32), "multistep and adaptive"), (dict(method=3), "multistep and adaptive"), (dict(thr=-0.5), ">= 0"),
                         (dict(thr=float("nan")), ">= 0"), (dict(coef=(C.c_double * 5)(0, 0, 0, float("inf"), 0)), "not finite")):
        assert centry(**kwargs) != 0 and word in eng.lib.lt_last_error().decode(), eng.lib.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # a run / reuse that does not follow its probe; a reuse without a residual; a reuse after the prompt was prepared again
    eng.forward_cached(z, t, "probe", use_cfg=True, **args)
    eng.forward(z, t, use_cfg=True, **args)
    for mode in ("run", "reuse"):
        with pytest.raises(_lib.LuminaLibError, match="does not follow its probe|without a stored residual"):
            eng.forward_cached(z, t, mode, use_cfg=True, **args)
    eng.forward_cached(z, t, "probe", use_cfg=True, **args)
    eng.forward_cached(z, t, "run", use_cfg=True, **args)
    eng.forward_cached(z, t, "probe", use_cfg=True, **args)
    eng.forward_cached(z, t, "reuse", use_cfg=True, **args)  # served
    eng._prompt.clear()
    eng.prepare_prompt(cap, cmask)  # lt_prepare_prompt forgets the residual
    eng.forward_cached(z, t, "probe", use_cfg=True, **args)
    with pytest.raises(_lib.LuminaLibError, match="without a stored residual"):
        eng.forward_cached(z, t, "reuse", use_cfg=True, **args)
    z2 = torch.cat([z, z])
    with pytest.raises(_lib.LuminaLibError, match="max_batch 2"):
        eng.forward_cached(z2, torch.cat([t, t]), "probe", use_cfg=True, **args)
    # MoE routing record
    moe, mcond, _, _ = _family(golden_dir, "moe")
    mkw = _kw(moe, mcond, "moe")
    meng, margs = moe._engine_sampler_args(z, True, dict(mkw))
    meng.moe_routing_record(True)
    try:
        with pytest.raises(_lib.LuminaLibError, match="MoE routing record"):
            meng.sample_ode_cached(z, o.t, "euler", use_cfg=True, threshold=0.1, **margs)
    finally:
        meng.moe_routing_record(False)
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW), ref)


# ---- 9. driver ---------------------------------------------------------------------------------------------------------------------------
def test_sample_driver_with_teacache_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    cfg, sd, _ = _deep(golden_dir, "next")
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_teacache_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_teacache_test"] = ctor
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

    argv = ["--ckpt", str(ck), "--caption_path", str(tmp_path / "prompts.txt"), "--resolution", "256:128x128", "--num_sampling_steps", "7",
            "--sampling-method", "euler", "--time_shifting_factor", "4", "--seed", "11"]
    runs = {}
    try:
        for name, extra in (("default", []), ("zero", ["--teacache", "0"]), ("huge", ["--teacache", "1e30"])):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            e = built[-1]._engine
            runs[name] = (e.last_nfe(), e.last_eval_rows(), e.last_cache_hits() if name != "default" else 0)
        with pytest.raises(SystemExit, match="cfg_reuse"):
            S.run(S.build_parser().parse_args(argv + ["--teacache", "0.1", "--cfg_reuse", "2", "--image_save_path", str(tmp_path / "no")]),
                  encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
    finally:
        del models.__dict__["NextDiT_tiny_teacache_test"]
    # every evaluation of a run lies in ONE whole-trajectory call
    assert runs == {"default": (6, 12, 0), "zero": (6, 12, 0), "huge": (6, 4, 4)}
    assert torch.equal(decoded[0], decoded[1]) and not torch.equal(decoded[2], decoded[0])
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    feats, mask = encode(["a red cube", ""])
    fn = Sampler(create_transport()).sample_ode(sampling_method="euler", num_steps=7, time_shifting_factor=4.0)
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    want = fn(z, model.forward_with_cfg, teacache=1e30, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1]
    assert torch.equal(decoded[2], want / 0.13025)
