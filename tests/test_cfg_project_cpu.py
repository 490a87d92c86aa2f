"""CPU: projected guidance - transport/guidance.py: guided_project / sample_cfg_project / check_project.  No GPU.

* APG at ``eta = 1, momentum = 0, r = inf`` is plain guidance ``bf16(c + fp32((w - 1) bf16(c - u)))`` word for word;
* at ``eta = 0`` the update is orthogonal to ``c`` up to the two fp32 roundings of its coefficients;
* the norm threshold clips ``m`` to ``r`` where ``|m| > r`` and leaves it alone elsewhere; the momentum is ``d2 + beta d1`` word for word;
* CFG-Zero* on collinear rows gives ``c`` whatever the scale; zero-init copies the state and calls the model less often;
* the checks, the driver's flags, the headers and the refusals that need no device."""
import math

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE

STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
INF = math.inf


def _rows(B, C, H, W, seed, amps=(0.25, 1.0, 4.0)):
    """cond rows of unit scale, uncond row b scaled by amps[b]: |c - u| spans a norm threshold between the samples"""
    g = torch.Generator().manual_seed(seed)
    half = B // 2
    cond = torch.randn(half, C, H, W, generator=g)
    unc = torch.randn(half, C, H, W, generator=g) * torch.tensor([amps[b % len(amps)] for b in range(half)]).view(-1, 1, 1, 1)
    return torch.cat([cond, unc]).to(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Toy:
    """a model with forward / forward_with_cfg on [B, 4, H, W] states that counts its calls"""
    cfg_channels = 3

    def __init__(self):
        self.calls = 0

    def forward(self, x, t, y):
        self.calls += 1
        s = (y.view(-1, 1, 1, 1).to(x.dtype) + 1.0)
        return (torch.sin(x.float() * 3.0 + t.view(-1, 1, 1, 1)) * s.float()).to(x.dtype) + x * 0.25

    def forward_with_cfg(self, x, t, y, cfg_scale):
        half = x[: len(x) // 2]
        o = self.forward(torch.cat([half, half]), t, y)
        c, u = o[: len(o) // 2], o[len(o) // 2:]
        g = u[:, :3] + cfg_scale * (c[:, :3] - u[:, :3])
        return torch.cat([torch.cat([g, c[:, 3:]], 1), torch.cat([g, u[:, 3:]], 1)])


@pytest.mark.parametrize("ch", [3, 4])
def test_apg_at_eta_one_without_momentum_or_threshold_is_plain_guidance_in_its_own_rounding_chain(ch):
    o = _rows(6, 4, 6, 10, seed=51)
    c, u = o[:3, :ch], o[3:, :ch]
    for w in (0.0, 4.0, 7.5, -1.5):
        got, coef, m = G.guided_project(o, w, ch, "apg")
        d = c - u  # bf16
        w1 = float(np.float32(np.float64(np.float32(w)) - 1.0))
        want = (c.float() + w1 * d.float()).to(torch.bfloat16)
        assert coef[:, 0].tolist() == [w1] * 3 and coef[:, 1].tolist() == [0.0] * 3
        assert torch.equal(_bits(m), _bits(d.float()))
        assert torch.equal(_bits(got[:3, :ch]), _bits(want)) and torch.equal(got[:3, :ch], got[3:, :ch]), w
        assert torch.equal(got[:, ch:], o[:, ch:])  # the channels past ch pass through row by row


def test_eta_zero_leaves_an_update_orthogonal_to_c_within_two_fp32_roundings():
    """With eta = 0 the update is a m + b c, a = fl((w - 1) tn), b = fl(-(w - 1) p), p = tn Smc / Scc.  In exact arithmetic
    a Smc + b Scc = (w - 1) tn Smc - (w - 1) tn Smc = 0.  Each coefficient carries one fp32 rounding, relative 2^-24, on top of float64 scalar
    arithmetic (a few 2^-53, negligible beside it): |a Smc + b Scc| <= 2^-24 |a Smc| + 2^-24 |b Scc| + (float64 terms) <= 2^-23 |a Smc| (1 + 2^-20),
    since |b Scc| = |a Smc| up to those roundings."""
    o = _rows(6, 4, 6, 10, seed=52)
    prev = torch.randn(3, 3, 6, 10, generator=torch.Generator().manual_seed(5))
    for w in (4.0, 7.5, -1.5):
        for r in (INF, 9.0):
            parts = []
            got, coef, m = G.guided_project(o, w, 3, "apg", eta=0.0, momentum=0.5, norm_threshold=r, m_prev=prev, parts=parts)
            for (Smm, Smc, Scc, tn, p), (a, b) in zip(parts, coef.tolist()):
                resid, scale = abs(a * Smc + b * Scc), abs(a * Smc)
                print(f"w {w} r {r}: |a Smc + b Scc| {resid:.3e}, bound {2.0 ** -23 * scale * (1 + 2.0 ** -20):.3e}")
                assert resid <= 2.0 ** -23 * scale * (1.0 + 2.0 ** -20), (w, r, resid, scale)


def test_norm_threshold_clips_the_samples_above_it_to_r_and_leaves_the_others():
    o = _rows(6, 4, 6, 10, seed=53)
    parts = []
    G.guided_project(o, 4.0, 3, "apg", parts=parts)
    norms = [math.sqrt(p[0]) for p in parts]
    assert min(norms) * 1.05 < max(norms)
    r = float(np.float32(math.sqrt(min(norms) * max(norms))))
    parts = []
    G.guided_project(o, 4.0, 3, "apg", norm_threshold=r, parts=parts)
    clipped = 0
    for Smm, _, _, tn, _ in parts:
        if math.sqrt(Smm) > r:
            clipped += 1
            assert tn < 1.0 and abs(tn * math.sqrt(Smm) - r) <= 2.0 ** -52 * r, (tn, Smm, r)  # one division, one product: an ulp of r
        else:
            assert tn == 1.0
    assert 0 < clipped < len(parts)


def test_momentum_over_two_evaluations_is_d2_plus_beta_d1_word_for_word():
    o1, o2 = _rows(4, 4, 6, 10, seed=54), _rows(4, 4, 6, 10, seed=55)
    for beta in (0.75, -0.5):
        _, _, m1 = G.guided_project(o1, 4.0, 3, "apg", momentum=beta)
        _, _, m2 = G.guided_project(o2, 4.0, 3, "apg", momentum=beta, m_prev=m1)
        d1, d2 = (o1[:2, :3] - o1[2:, :3]).float(), (o2[:2, :3] - o2[2:, :3]).float()
        assert m1.dtype == torch.float32 and torch.equal(_bits(m1), _bits(d1))
        b = np.float32(beta)
        want = (d2.numpy() + (b * d1.numpy()).astype(np.float32)).astype(np.float32)
        assert np.array_equal(m2.numpy().view(np.int32), want.view(np.int32)) and not torch.equal(m2, d2)


def test_zero_star_on_collinear_rows_gives_c_whatever_the_scale():
    c = torch.randn(3, 4, 6, 10, generator=torch.Generator().manual_seed(56)).to(torch.bfloat16)
    for k in (0.25, 2.0, -4.0):
        o = torch.cat([c, (c.float() * k).to(torch.bfloat16)])  # a power of two: exact in bf16
        for w in (0.0, 4.0, 7.5, -1.5):
            got, s, m = G.guided_project(o, w, 3, "zero_star")
            assert m is None and s.tolist() == [1.0 / k] * 3, (k, s.tolist())
            assert torch.equal(_bits(got[:3, :3]), _bits(c[:, :3])) and torch.equal(got[3:, :3], got[:3, :3]), (k, w)
            assert torch.equal(got[:, 3:], o[:, 3:])
    got, s, _ = G.guided_project(torch.cat([c, torch.zeros_like(c)]), 4.0, 3, "zero_star")  # <u, u> = 0: s = 1, g = w c
    assert s.tolist() == [1.0] * 3 and bool(torch.isfinite(got.float()).all())


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_zero_init_copies_the_state_and_calls_the_model_less_often(method):
    tgrid = ODE(6, method, 4).t
    st = STAGES[method]
    z = torch.randn(1, 4, 4, 4, generator=torch.Generator().manual_seed(57)).repeat(2, 1, 1, 1)
    y = torch.tensor([1.0, 0.0])
    table = torch.tensor([1.5 + 0.5 * (i % 4) for i in range(5 * st)])
    table[st] = 1.0  # a conditional-only stage
    full = None
    for K in (0, 1, 3):
        toy, calls = Toy(), []
        out = G.sample_cfg_project(toy, z, tgrid, table, method, zero_star=True, zero_init=K, calls=calls, y=y)
        assert toy.calls == (6 - 1 - K) * st and calls == [toy.calls]
        for i in range(K + 1):
            assert torch.equal(out[i], z)
        assert not torch.equal(out[K + 1], z)
        if K == 0:
            full = out
        # through the front end, a model that is not engine-backed runs the same host loop
        toy2 = Toy()
        assert torch.equal(ODE(6, method, 4).sample(z, toy2.forward_with_cfg, cfg_table=table, cfg_zero_star=True, cfg_zero_init=K, y=y), out)
        assert toy2.calls == toy.calls
    assert not torch.equal(out[-1], full[-1])
    with pytest.raises(ValueError, match="zero_init"):
        G.sample_cfg_project(Toy(), z, tgrid, table, method, zero_star=True, zero_init=5, y=y)
    # APG through the loop: the momentum advances with the guided stages only, in evaluation order
    parts, factors = [], []
    G.sample_cfg_project(Toy(), z, tgrid, table, method, apg=dict(eta=0.5, momentum=0.5), parts=parts, factors=factors, y=y)
    assert len(factors) == int((table != 1).sum()) == len(parts)


def test_checks_refusals_and_the_driver_flags():
    assert G.check_project() == (None, 1.0, 0.0, INF, 0)
    assert G.check_project(zero_star=True, zero_init=2) == ("zero_star", 1.0, 0.0, INF, 2)
    form, eta, beta, r, K = G.check_project(dict(eta=0.1, momentum=-0.3))
    assert form == "apg" and eta == float(np.float32(0.1)) and beta == float(np.float32(-0.3)) and r == INF and K == 0
    for bad, word in ((dict(eta=float("nan")), "eta"), (dict(eta=INF), "eta"), (dict(momentum=1.0), "momentum"), (dict(momentum=-1.0), "momentum"),
                      (dict(momentum=float("nan")), "momentum"), (dict(norm_threshold=0.0), "norm_threshold"),
                      (dict(norm_threshold=-1.0), "norm_threshold"), (dict(norm_threshold=float("nan")), "norm_threshold"), (dict(beta=0.5), "beta")):
        with pytest.raises(ValueError, match=word):
            G.check_project(bad)
    with pytest.raises(ValueError, match="exclusive"):
        G.check_project(dict(eta=0.5), zero_star=True)
    for K in (1, -1, 1.5, True):
        with pytest.raises(ValueError, match="zero_init"):
            G.check_project(None, K is True, K) if K is not True else G.check_project(None, True, True)
    with pytest.raises(ValueError, match="zero_init"):
        G.check_project(None, True, 4, n_grid=5)
    assert G.check_project(None, True, 3, n_grid=5)[4] == 3
    G.refuse_with_project(None, "abm2", 0.5, 1.0, [0], [0.5], [0.5], 0.1, object(), True)  # off: nothing to refuse
    for k, word in ((dict(rescale=0.5), "rescale / norm_limit"), (dict(norm_limit=1.0), "rescale / norm_limit"), (dict(reuse=[0, 1]), "reuse"),
                    (dict(slg=[0.5]), "skip-layer"), (dict(pag=[0.5]), "perturbed-attention"), (dict(teacache=0.1), "teacache"),
                    (dict(mask=object()), "mask"), (dict(packed=True), "packed"), (dict(method="abm2"), "fixed-grid"),
                    (dict(method="ab3"), "fixed-grid"), (dict(method="dopri5"), "fixed-grid")):
        for form in ("apg", "zero_star"):
            with pytest.raises(ValueError, match=word):
                G.refuse_with_project(form, **k)
    o = _rows(4, 4, 2, 2, seed=1)
    with pytest.raises(ValueError, match="even batch"):
        G.guided_project(o[:3], 4.0, 3, "apg")
    with pytest.raises(ValueError, match="form"):
        G.guided_project(o, 4.0, 3, "apg2")
    toy, z, y = Toy(), torch.zeros(2, 4, 2, 2), torch.ones(2)
    ode = ODE(3, "euler")
    with pytest.raises(ValueError, match="exclusive"):
        ode.sample(z, toy.forward_with_cfg, cfg_apg=dict(eta=0.5), cfg_zero_star=True, y=y, cfg_scale=4.0)
    with pytest.raises(ValueError, match="rescale / norm_limit"):
        ode.sample(z, toy.forward_with_cfg, cfg_apg=dict(eta=0.5), cfg_rescale=0.5, y=y, cfg_scale=4.0)
    with pytest.raises(ValueError, match="mask"):
        ode.sample(z, toy.forward_with_cfg, cfg_zero_star=True, mask=torch.ones_like(z), x1=z, noise=z, y=y, cfg_scale=4.0)
    with pytest.raises(ValueError, match="fixed-grid"):
        ODE(3, "abm2").sample(z, toy.forward_with_cfg, cfg_zero_star=True, y=y, cfg_scale=4.0)
    with pytest.raises(ValueError, match="a projected form"):
        G.sample_cfg_project(toy, z, ode.t, [4.0, 4.0], "euler", y=y)
    assert toy.calls == 0
    # without a table: cfg_scale at every stage
    got = ode.sample(z + 0.5, toy.forward_with_cfg, cfg_zero_star=True, y=y, cfg_scale=4.0)
    assert torch.equal(got, G.sample_cfg_project(Toy(), z + 0.5, ode.t, [4.0, 4.0], "euler", zero_star=True, y=y))

    from lumina_t2x_amd import sample as S
    args = S.build_parser().parse_args(["--ckpt", "nowhere"])
    assert args.apg_eta is None and args.apg_momentum is None and args.apg_norm_threshold is None
    assert args.cfg_zero_star is False and args.cfg_zero_init == 0 and S.guidance_project(args) == {}  # run() then makes the call it made before
    args = S.build_parser().parse_args(["--ckpt", "nowhere", "--apg_eta", "0.25", "--apg_momentum", "-0.5", "--cfg_interval", "0.1", "0.8"])
    assert S.guidance_project(args) == dict(cfg_apg=dict(eta=0.25, momentum=-0.5, norm_threshold=INF))
    assert S.guidance_table(args, ODE(5, "euler").t) is not None
    args = S.build_parser().parse_args(["--ckpt", "nowhere", "--apg_norm_threshold", "2.5", "--cfg_schedule", "linear"])
    assert S.guidance_project(args) == dict(cfg_apg=dict(eta=1.0, momentum=0.0, norm_threshold=2.5))
    args = S.build_parser().parse_args(["--ckpt", "nowhere", "--cfg_zero_star", "--cfg_zero_init", "2"])
    assert S.guidance_project(args) == dict(cfg_zero_star=True, cfg_zero_init=2)
    for argv, word in ((["--apg_eta", "0.5", "--cfg_zero_star"], "exclusive"), (["--cfg_zero_init", "2"], "zero_init"),
                       (["--apg_momentum", "1.0"], "momentum"), (["--apg_norm_threshold", "0"], "norm_threshold"),
                       (["--cfg_zero_star", "--sampling-method", "abm2"], "fixed-grid"), (["--apg_eta", "0.5", "--solver", "dopri5"], "fixed-grid")):
        with pytest.raises(SystemExit, match=word):
            S.guidance_project(S.build_parser().parse_args(["--ckpt", "nowhere"] + argv))


def test_headers_declare_the_entries_and_argument_errors_come_back_by_name_without_a_device():
    import ctypes as C
    lib = _lib.load()
    for name in ("lt_sample_ode_cfg_project", "lt_forward_cfg_project", "lt_op_guidance_project_stats", "lt_op_unpatchify_cfg_project"):
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(lib, name), name
    assert (_lib.LT_PROJECT_APG, _lib.LT_PROJECT_ZERO_STAR) == (1, 2) and _lib.PROJECT_FORMS == G.PROJECT_FORMS
    a = _lib.LtStepArgs(batch=2, io_dtype=_lib.LT_BF16)
    grid = (C.c_float * 2)(0.0, 1.0)
    one = C.c_void_p(64)  # never dereferenced: every call below is refused before it reads anything
    assert lib.lt_sample_ode_cfg_project(one, one, None, one, grid, 2, 0, None, 1, 0.5, 0.5, 1.0, 0, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_cfg_project: null argument" in lib.lt_last_error()
    assert lib.lt_forward_cfg_project(None, one, one, one, 1, 0.5, 0.5, 1.0, 0, C.byref(a), None) != 0
    assert b"lt_forward_cfg_project: null argument" in lib.lt_last_error()
    assert lib.lt_op_guidance_project_stats(one, 40, 3, 8, 6, 10, 2, 3, 0, 1, one, one, one, None) != 0 and b"even" in lib.lt_last_error()
    assert lib.lt_op_guidance_project_stats(one, 40, 2, 8, 6, 10, 2, 3, 0, 3, one, one, one, None) != 0 and b"form" in lib.lt_last_error()
    assert lib.lt_op_guidance_project_stats(one, 40, 2, 8, 6, 10, 2, 3, 0, 1, one, None, one, None) != 0 and b"momentum" in lib.lt_last_error()
    assert lib.lt_op_unpatchify_cfg_project(one, 40, one, 1, 1024, 4, 8, 6, 10, 2, 1, one, 3, 0, 0, 1, one, one, one, None, None) != 0
    assert b"256" in lib.lt_last_error()
    assert lib.lt_op_unpatchify_cfg_project(one, 40, one, 1, 2, 4, 8, 6, 10, 2, 1, one, 3, 0, 0, 0, one, one, one, None, None) != 0
    assert b"form" in lib.lt_last_error()
