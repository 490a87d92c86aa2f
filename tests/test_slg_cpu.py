"""CPU: skip-layer guidance - the definition ``transport.guidance.sample_cfg_slg``, its chain of roundings, the table builder, the
Python-level refusals, the driver's flags and the ABI declarations.  Everything is exact: no tolerance.

The package has no torch forward pass (every family runs on the engine), so "forward(skip_layers=S) equals the model with those blocks
removed" is checked where the families run: tests/test_gpu_slg.py, against a model rebuilt without the blocks.  Here the same property is held
on the toy model the loop tests use."""
import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE

import exact_slg as X
from exact_reuse import f64, same_bits

STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
NEW = ("lt_forward_skip", "lt_forward_cfg_slg", "lt_sample_ode_cfg_slg", "lt_op_unpatchify_cfg_slg")


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1.5, 2.5, -4.5])
@pytest.mark.parametrize("w", [1.5, 2.5, 4.5])
def test_chain_on_bf16_ties_equals_the_float64_restatement(w, s):
    c, u, k = X.tie_operands(w, s)
    cf, uf, kf = f64(c), f64(u), f64(k)
    # the operands do what they were built for: ties in both products and in both sums
    wd = np.float64(np.float32(w)) * (cf - uf)
    se = np.float64(np.float32(s)) * (cf - kf)
    g0 = X.bf16_round64(uf + X.bf16_round64(wd))
    assert X.count_ties(wd) > 0 and X.count_ties(se) > 0
    assert X.count_ties(uf + X.bf16_round64(wd)) > 0
    if s > 0:  # (terms of opposite sign cancel the high bits: the sum is then exact in bf16, which the comparison below covers all the same)
        assert X.count_ties(g0 + X.bf16_round64(se)) > 0
    got = G.slg_combine(c, u, k, w, s)
    assert got.dtype == torch.bfloat16 and same_bits(got, X.slg_chain(cf, uf, kf, w, s))
    got1 = G.slg_combine(c, None, k, 1.0, s)
    assert same_bits(got1, X.slg_chain(cf, None, kf, 1.0, s))
    assert X.count_ties(cf + X.bf16_round64(se)) > 0


@pytest.mark.parametrize("s", [2.8, -1.0, 1e30])
def test_chain_with_skip_equal_to_cond_has_no_slg_term(s):
    g = torch.Generator().manual_seed(2)
    c = torch.randn(4096, generator=g).mul(3).to(torch.bfloat16)
    u = torch.randn(4096, generator=g).mul(3).to(torch.bfloat16)
    got = G.slg_combine(c, u, c.clone(), 4.0, s)
    assert same_bits(got, X.slg_chain(f64(c), f64(u), f64(c), 4.0, s))
    assert torch.equal(got, u + 4.0 * (c - u))  # s * 0 = 0, and x + 0 = x
    assert torch.equal(G.slg_combine(c, None, c.clone(), 1.0, s), c)


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def test_slg_table_interval_edges_empty_interval_and_refusals():
    tgrid = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])
    assert G.slg_table(tgrid, "euler", 2.8).tolist() == [pytest.approx(2.8)] * 4
    # lo <= t < hi on the unrounded stage times: 0.25 is in, 0.75 is out
    assert G.slg_table(tgrid, "euler", 2.0, interval=(0.25, 0.75)).tolist() == [0.0, 2.0, 2.0, 0.0]
    mid = G.slg_table(tgrid, "midpoint", 2.0, interval=(0.25, 0.75)).tolist()  # stage times 0, .125, .25, .375, .5, .625, .75, .875
    assert mid == [0.0, 0.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0]
    assert G.slg_table(tgrid, "rk4", 2.0, interval=(0.5, 0.5)).tolist() == [0.0] * 16  # an empty interval
    assert G.slg_table(tgrid, "rk4", 2.0).dtype == torch.float32
    with pytest.raises(ValueError, match="not ordered"):
        G.slg_table(tgrid, "euler", 2.0, interval=(0.6, 0.4))
    with pytest.raises(ValueError, match="not finite"):
        G.slg_table(tgrid, "euler", float("inf"))
    with pytest.raises(ValueError, match="fixed-grid"):
        G.slg_table(tgrid, "dopri5", 2.0)
    with pytest.raises(ValueError, match="3 entries"):
        G.check_slg([1.0, 2.0, 3.0], tgrid, "euler")
    with pytest.raises(ValueError, match="not finite"):
        G.check_slg([1.0, float("nan"), 3.0, 0.0], tgrid, "euler")
    with pytest.raises(ValueError, match="is None"):
        G.check_slg(None, tgrid, "euler")
    assert G.check_slg_layers([7, 8, 9]) == [7, 8, 9] and G.check_slg_layers(torch.tensor([2, 0]), 3) == [2, 0]
    for bad, word in (([1, 1], "repeated"), ([1.5], "not an integer"), ([True], "not an integer")):
        with pytest.raises(ValueError, match=word):
            G.check_slg_layers(bad)
    for bad, word in (([3], "outside 0..2"), ([-1], "outside 0..2"), ([0, 1, 2], "leaves no layer")):
        with pytest.raises(ValueError, match=word):
            G.check_slg_layers(bad, 3)


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
class Toy:
    """a torch 'model' of three residual blocks with a bf16 output: forward (with skip_layers), and the reference's forward_with_cfg"""
    cfg_channels = 3
    n_layers = 3

    def __init__(self, layers=(0, 1, 2)):
        self.layers = list(layers)  # which of the three block functions this model holds, in order
        self.n_layers = len(self.layers)
        self.seen = []

    @staticmethod
    def block(i, h, t, y):
        a = (0.5, -0.75, 0.25)[i]
        return h + torch.tanh(h * (a * y)) * (t + 0.5 * i)

    def net(self, x, t, y, skip=()):
        h = x.to(torch.bfloat16)
        yv, tv = y.view(-1, 1, 1, 1).to(h.dtype), t.view(-1, 1, 1, 1).to(h.dtype)
        for pos, i in enumerate(self.layers):
            if pos not in skip:
                h = self.block(i, h, tv, yv)
        return h - tv * x.to(torch.bfloat16)

    def forward(self, x, t, y, skip_layers=()):
        assert t.dtype == torch.float32 and t.shape[0] == x.shape[0] == y.shape[0]
        self.seen.append((x.shape[0], tuple(skip_layers)))
        return self.net(x, t, y, tuple(skip_layers)).to(x.dtype)

    def forward_with_cfg(self, x, t, y, cfg_scale):
        half = x[: len(x) // 2]
        out = self.net(torch.cat([half, half]), t, y)
        eps, rest = out[:, :3], out[:, 3:]
        cond, unc = eps.chunk(2)
        g = unc + cfg_scale * (cond - unc)
        return torch.cat([torch.cat([g, g]), rest], dim=1).to(x.dtype)


def _state(dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(2, 4, 6, 10, generator=g).to(dtype).repeat(2, 1, 1, 1)
    y = torch.tensor([0.5, 1.5, -0.75, 0.25])
    return z, y


@pytest.mark.parametrize("S", [(1,), (0,), (2,), (0, 1), (1, 2)])
def test_toy_forward_with_skip_layers_equals_the_model_without_those_blocks(S):
    z, y = _state(torch.bfloat16)
    t = torch.full((4,), 0.375)
    full, cut = Toy(), Toy([i for i in range(3) if i not in S])
    assert torch.equal(full.forward(z, t, y, skip_layers=S), cut.forward(z, t, y))
    assert not torch.equal(full.forward(z, t, y, skip_layers=S), full.forward(z, t, y))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_all_zero_slg_table_is_the_schedule_loop_bit_for_bit(method, dtype):
    z, y = _state(dtype)
    tgrid = ODE(5, method, 4).t
    n = 4 * STAGES[method]
    table = torch.tensor([[4.0, 1.0, 2.5, 7.5, 1.0, -1.0, 3.0, 0.0][i % 8] for i in range(n)])
    want = G.sample_cfg_schedule(Toy(), z, tgrid, table, method, y=y)
    toy = Toy()
    got = G.sample_cfg_slg(toy, z, tgrid, table, [0.0] * n, [1], method, y=y)
    assert got.dtype == dtype and torch.equal(got, want)
    assert all(skip == () for _, skip in toy.seen)  # no skip evaluation was made
    # through the transport front end
    assert torch.equal(ODE(5, method, 4).sample(z, Toy().forward_with_cfg, cfg_table=table, slg_table=[0.0] * n, slg_layers=[1], y=y,
                                                cfg_scale=9.0), want)
    # ... and a stage with s != 0 changes the trajectory, with one more evaluation of the cond rows, blocks left out
    slg = G.slg_table(tgrid, method, 2.8, interval=(0.0, float(tgrid[2])))  # the stages of the first two steps
    m = int((slg != 0).sum())
    assert 0 < m < n
    toy = Toy()
    other = G.sample_cfg_slg(toy, z, tgrid, table, slg, [1], method, y=y)
    assert not torch.equal(other, want) and bool(torch.isfinite(other.float()).all())
    assert sum(1 for rows, skip in toy.seen if skip == (1,)) == m and all(rows == 2 for rows, skip in toy.seen if skip)
    assert torch.equal(ODE(5, method, 4).sample(z, Toy().forward_with_cfg, cfg_table=table, slg_table=slg, slg_layers=[1], y=y), other)


@pytest.mark.parametrize("w", [4.0, 1.0])
def test_one_stage_equals_the_float64_restatement(w):
    z, y = _state(torch.bfloat16)
    tgrid = torch.tensor([0.25, 0.5])
    toy = Toy()
    got = G.sample_cfg_slg(toy, z, tgrid, [w], [2.5], [0, 2], "euler", y=y, t_round=False)
    t = torch.full((4,), 0.25)
    o = toy.net(torch.cat([z[:2]] * 2), t, y)
    k = toy.net(z[:2], t[:2], y[:2], skip=(0, 2))
    g = X.slg_chain(f64(o[:2, :3]), None if w == 1.0 else f64(o[2:, :3]), f64(k[:, :3]), w, 2.5)
    slope = (got[1].float() - z.float()) / 0.25  # euler: y1 = y0 + dt * slope, dt = 0.25 exactly; recover the slope where that is exact
    want = torch.from_numpy(np.asarray(g)).to(torch.bfloat16)
    step = (z[:2, :3] + torch.tensor(0.25) * want).to(torch.bfloat16)
    assert torch.equal(got[1][:2, :3], step) and torch.equal(got[1][2:, :3], step)
    assert slope.shape == z.shape
    rest = o[:2, 3:] if w == 1.0 else o[2:, 3:]
    assert torch.equal(got[1][2:, 3:], (z[2:, 3:] + torch.tensor(0.25) * rest).to(torch.bfloat16))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_python_layer_refusals():
    z, y = _state(torch.bfloat16)
    tgrid = ODE(5, "euler", 4).t
    fours, twos = [4.0] * 4, [2.0] * 4
    with pytest.raises(ValueError, match="rescale / norm_limit"):
        G.sample_cfg_slg(Toy(), z, tgrid, fours, twos, [1], "euler", y=y, rescale=0.5)
    with pytest.raises(ValueError, match="rescale / norm_limit"):
        ODE(5, "euler", 4).sample(z, Toy().forward_with_cfg, cfg_table=fours, slg_table=twos, slg_layers=[1], cfg_norm_limit=1.5, y=y)
    with pytest.raises(ValueError, match="guidance reuse"):
        ODE(5, "euler", 4).sample(z, Toy().forward_with_cfg, cfg_table=fours, slg_table=twos, slg_layers=[1], cfg_reuse=[0, 1, 0, 1], y=y)
    with pytest.raises(ValueError, match="packed batch"):
        G.sample_cfg_slg(Toy(), [z[:1], z[:1]], tgrid, fours, twos, [1], "euler", y=y)
    with pytest.raises(ValueError, match="packed batch"):
        ODE(5, "euler", 4).sample([z[:1], z[:1]], Toy().forward_with_cfg, cfg_table=fours, slg_table=twos, slg_layers=[1], y=y)
    with pytest.raises(NotImplementedError, match="inpainting mask"):
        ODE(5, "euler", 4).sample(z, Toy().forward_with_cfg, mask=torch.ones(6, 10), x1=z, noise=z, slg_table=twos, slg_layers=[1], y=y)
    with pytest.raises(ValueError, match="even batch"):
        G.sample_cfg_slg(Toy(), z[:3], tgrid, fours, twos, [1], "euler", y=y[:3])
    for method in ("abm2", "dopri5"):
        with pytest.raises(ValueError, match="fixed-grid"):
            G.sample_cfg_slg(Toy(), z, tgrid, fours, twos, [1], method, y=y)
    with pytest.raises((ValueError, NotImplementedError), match="fixed-grid"):
        ODE(5, "abm2", 4).sample(z, Toy().forward_with_cfg, cfg_table=fours, slg_table=twos, slg_layers=[1], y=y)
    with pytest.raises(ValueError, match="3 entries"):
        G.sample_cfg_slg(Toy(), z, tgrid, fours, twos[:3], [1], "euler", y=y)
    with pytest.raises(ValueError, match="not finite"):
        G.sample_cfg_slg(Toy(), z, tgrid, fours, [2.0, float("nan"), 0.0, 0.0], [1], "euler", y=y)
    with pytest.raises(ValueError, match="is None"):
        G.sample_cfg_slg(Toy(), z, tgrid, fours, None, [1], "euler", y=y)
    for bad, word in (([3], "outside 0..2"), ([1, 1], "repeated"), ([0, 1, 2], "leaves no layer")):
        with pytest.raises(ValueError, match=word):
            G.sample_cfg_slg(Toy(), z, tgrid, fours, twos, bad, "euler", y=y)
    # rule parameters at their defaults are no rule
    got = G.sample_cfg_slg(Toy(), z, tgrid, fours, twos, [1], "euler", y=y, rescale=0.0, norm_limit=float("inf"))
    assert torch.equal(got, G.sample_cfg_slg(Toy(), z, tgrid, fours, twos, [1], "euler", y=y))


def test_sample_driver_flags():
    from lumina_t2x_amd import sample as S
    p = S.build_parser()
    base = ["--ckpt", "x", "--sampling-method", "midpoint"]
    tgrid = ODE(5, "midpoint", 4).t
    d = p.parse_args(base)
    assert d.slg_layers is None and d.slg_scale == 0.0 and d.slg_interval is None
    assert S.guidance_slg(d, tgrid) is None  # the default: the call it was
    assert S.guidance_slg(p.parse_args(base + ["--slg_layers", "7", "8", "9"]), tgrid) is None  # scale 0: off
    on = base + ["--slg_layers", "7", "8", "9", "--slg_scale", "2.8"]
    assert torch.equal(S.guidance_slg(p.parse_args(on), tgrid), G.slg_table(tgrid, "midpoint", 2.8))
    got = S.guidance_slg(p.parse_args(on + ["--slg_interval", "0.01", "0.2"]), tgrid)
    assert torch.equal(got, G.slg_table(tgrid, "midpoint", 2.8, interval=(0.01, 0.2))) and 0 < int((got != 0).sum()) < 8
    # combines with the guidance interval / schedule
    args = p.parse_args(on + ["--cfg_interval", "0.1", "0.8", "--cfg_schedule", "linear"])
    assert S.guidance_table(args, tgrid) is not None and S.guidance_slg(args, tgrid) is not None
    for extra, word in ((["--cfg_rescale", "0.5"], "cfg_rescale"), (["--cfg_norm_limit", "1.5"], "cfg_norm_limit"),
                        (["--cfg_reuse", "2"], "cfg_reuse"), (["--cfg_reuse_per_step"], "cfg_reuse")):
        with pytest.raises(SystemExit, match=word):
            S.guidance_slg(p.parse_args(on + extra), tgrid)
    for method in ("abm2", "ab3", "dopri5"):
        with pytest.raises(SystemExit, match="sampling methods"):
            S.guidance_slg(p.parse_args(["--ckpt", "x", "--sampling-method", method] + on[4:]), tgrid)
    with pytest.raises(SystemExit, match="need --slg_layers"):
        S.guidance_slg(p.parse_args(base + ["--slg_scale", "2.8"]), tgrid)
    with pytest.raises(SystemExit, match="repeated"):
        S.guidance_slg(p.parse_args(base + ["--slg_layers", "7", "7", "--slg_scale", "2.8"]), tgrid)
    with pytest.raises(SystemExit, match="not ordered"):
        S.guidance_slg(p.parse_args(on + ["--slg_interval", "0.6", "0.2"]), tgrid)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_documented():
    declared = set(_lib.declared_symbols())
    text = _lib.header_text(strip_comments=False)
    for name in NEW:
        assert name in declared and name in _lib._SIGNATURES, name
    for word in ("skip_host", "DESIGN.md 7m", "R(R(u + R(w R(c - u))) + R(s R(c - k)))", "five HIP-graph keys"):
        assert word in text, word
