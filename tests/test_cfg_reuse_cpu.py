"""CPU: guidance reuse - transport/guidance.py: cfg_reuse_table / check_reuse / sample_cfg_reuse.  No GPU.  Everything is exact.

* ``cfg_reuse_table``: ``every``, ``interval``, ``per_step``; scale-1 entries are 0; the first guided entry is a refresh; refusals;
* an all-zero flag table: ``sample_cfg_reuse`` IS ``sample_cfg_schedule`` around a torch toy model, bit for bit;
* a toy model whose cond - uncond does not depend on t or x: a reuse stage gives what the float64 restatement of the refresh chain's
  expression ``R(R(c - d) + R(w d))`` gives, to the last bit;
* the reuse chain against that restatement on operands that meet bf16 ties in ``w d`` and in the final sum;
* refusals of the Python layer; the ABI declares, binds and documents the new entries."""
import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE

import exact_reuse as X

STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
NEW = ("lt_sample_ode_cfg_reuse", "lt_sample_ode_multistep_cfg_reuse", "lt_forward_cfg_reuse", "lt_op_unpatchify_cfg_reuse")


# ---- the flag table ------------------------------------------------------------------------------------------------------------------
def test_table_every_counts_guided_evaluations_only():
    tgrid = ODE(5, "midpoint", 4).t
    table = torch.tensor([1.0, 4.0, 4.0, 1.0, 3.0, 4.0, 4.0, 1.0])
    assert G.cfg_reuse_table(tgrid, "midpoint", table).tolist() == [0, 0, 1, 0, 0, 1, 0, 0]
    assert G.cfg_reuse_table(tgrid, "midpoint", table, every=3).tolist() == [0, 0, 1, 0, 1, 0, 1, 0]
    assert G.cfg_reuse_table(tgrid, "midpoint", table, every=1).tolist() == [0] * 8
    flags = G.cfg_reuse_table(tgrid, "midpoint", table)
    assert flags.dtype == torch.int32 and bool((flags[table == 1] == 0).all())
    fours = torch.full((8,), 4.0)
    assert G.cfg_reuse_table(tgrid, "midpoint", fours).tolist() == [0, 1] * 4
    assert G.cfg_reuse_table(tgrid, "midpoint", fours, per_step=True).tolist() == [0, 1] * 4
    assert G.cfg_reuse_table(ODE(3, "rk4", 4).t, "rk4", fours, per_step=True).tolist() == [0, 1, 1, 1] * 2
    # per_step: the first GUIDED stage of an interval refreshes, wherever the interval's guidance opens
    assert G.cfg_reuse_table(tgrid, "midpoint", table, per_step=True).tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert G.cfg_reuse_table(ODE(5, "euler", 4).t, "ab2", [4.0, 4.0, 1.0, 4.0]).tolist() == [0, 1, 0, 0]


def test_table_interval_and_the_first_guided_entry():
    tgrid = ODE(5, "midpoint", 4).t
    ts = G.stage_times(tgrid, "midpoint", torch.float32, False).tolist()
    fours = torch.full((8,), 4.0)
    # reuse inside [ts[3], ts[7]): evaluations 3..6 are numbered 0..3, the guided ones outside refresh
    got = G.cfg_reuse_table(tgrid, "midpoint", fours, interval=(ts[3], ts[7])).tolist()
    assert got == [0, 0, 0, 0, 1, 0, 1, 0]
    # an interval whose first evaluation would be a reuse: the first guided evaluation of the trajectory refreshes all the same
    got = G.cfg_reuse_table(tgrid, "midpoint", torch.tensor([1.0] + [4.0] * 7), every=2, interval=(ts[0], ts[8 - 1] + 1.0)).tolist()
    assert got[0] == 0 and got[1] == 0
    G.check_reuse(got, torch.tensor([1.0] + [4.0] * 7), tgrid, "midpoint")
    # the table does not depend on the state dtype: the interval is taken on the unrounded stage times
    assert G.cfg_reuse_table(tgrid, "midpoint", fours, interval=(ts[1], ts[1] + 1e-6)).tolist() == [0] * 8


def test_table_and_flag_refusals():
    tgrid = ODE(5, "euler", 4).t
    with pytest.raises(ValueError, match="entries"):
        G.cfg_reuse_table(tgrid, "euler", [4.0] * 3)
    with pytest.raises(ValueError, match="every"):
        G.cfg_reuse_table(tgrid, "euler", [4.0] * 4, every=0)
    with pytest.raises(ValueError, match="not ordered"):
        G.cfg_reuse_table(tgrid, "euler", [4.0] * 4, interval=(0.8, 0.1))
    with pytest.raises(ValueError, match="fixed-grid"):
        G.cfg_reuse_table(tgrid, "dopri5", [4.0] * 4)
    with pytest.raises(ValueError, match="reuse table has 3 entries"):
        G.check_reuse([0, 1, 1], [4.0] * 4, tgrid, "euler")
    for bad in (2, -1, 0.5):
        with pytest.raises(ValueError, match="is not 0 .refresh. or 1 .reuse."):
            G.check_reuse([0, 1, bad, 0], [4.0] * 4, tgrid, "euler")
    with pytest.raises(ValueError, match="evaluation 0 reuses"):
        G.check_reuse([1, 0, 0, 0], [4.0] * 4, tgrid, "euler")
    with pytest.raises(ValueError, match="evaluation 1 reuses"):  # the refresh flag at scale 1 refreshes nothing
        G.check_reuse([0, 1, 0, 0], [1.0, 4.0, 4.0, 4.0], tgrid, "euler")
    table, flags = G.check_reuse(torch.tensor([1, 0, 1, True]), [1.0, 4.0, 4.0, 4.0], tgrid, "euler")  # a flag 1 at scale 1 is no reuse
    assert flags == [1, 0, 1, 1] and table.dtype == torch.float32


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
class Toy:
    """a torch 'model' with a bf16 output: forward, and the reference's forward_with_cfg (guidance on the first cfg_channels channels)"""
    cfg_channels = 3

    def net(self, x, t, y):
        xb = x.to(torch.bfloat16)
        return torch.tanh(xb * y.view(-1, 1, 1, 1).to(xb.dtype)) - t.view(-1, 1, 1, 1).to(xb.dtype) * xb

    def forward(self, x, t, y):
        assert t.dtype == torch.float32 and t.shape[0] == x.shape[0] == y.shape[0]
        return self.net(x, t, y).to(x.dtype)

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


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_all_refresh_table_is_the_schedule_loop_bit_for_bit(method, dtype):
    z, y = _state(dtype)
    tgrid = ODE(5, method, 4).t
    n = 4 * STAGES[method]
    table = torch.tensor([[4.0, 1.0, 2.5, 7.5, 1.0, -1.0, 3.0, 0.0][i % 8] for i in range(n)])
    want = G.sample_cfg_schedule(Toy(), z, tgrid, table, method, y=y)
    deltas = []
    got = G.sample_cfg_reuse(Toy(), z, tgrid, table, [0] * n, method, y=y, deltas=deltas)
    assert got.dtype == dtype and torch.equal(got, want) and len(deltas) == int((table != 1).sum())
    assert all(d.dtype == torch.bfloat16 and d.shape == (2, 3, 6, 10) for d in deltas)
    # through the transport front end, and flags that only sit on scale-1 stages change nothing
    assert torch.equal(ODE(5, method, 4).sample(z, Toy().forward_with_cfg, cfg_table=table, cfg_reuse=[0] * n, y=y, cfg_scale=9.0), want)
    assert torch.equal(G.sample_cfg_reuse(Toy(), z, tgrid, table, (table == 1).int(), method, y=y), want)
    # ... and a reuse stage changes the trajectory of this model, whose cond - uncond moves with t and x
    flags = G.cfg_reuse_table(tgrid, method, table)
    assert int(flags.sum()) > 0 and not torch.equal(G.sample_cfg_reuse(Toy(), z, tgrid, table, flags, method, y=y), want)


@pytest.mark.parametrize("method", ["ab2", "abm3"])
def test_all_refresh_table_is_the_multistep_schedule_loop_bit_for_bit(method):
    z, y = _state(torch.bfloat16)
    tgrid = ODE(7, "euler", 4).t
    table = torch.tensor([4.0, 1.0, 2.5, 7.5, 1.0, 3.0])
    want = G.sample_cfg_multistep(Toy(), z, tgrid, table, method, y=y)
    assert torch.equal(G.sample_cfg_reuse_multistep(Toy(), z, tgrid, table, [0] * 6, method, y=y), want)
    assert torch.equal(ODE(7, method, 4).sample(z, Toy().forward_with_cfg, cfg_table=table, cfg_reuse=[0] * 6, y=y), want)
    flags = [0, 0, 1, 1, 0, 1]
    got = G.sample_cfg_reuse_multistep(Toy(), z, tgrid, table, flags, method, y=y)
    assert not torch.equal(got, want)
    assert torch.equal(ODE(7, method, 4).sample(z, Toy().forward_with_cfg, cfg_table=table, cfg_reuse=flags, y=y), got)


class Shifted(Toy):
    """cond - uncond is one fixed bf16 field, whatever t and x are: the cond rows are the uncond rows' output plus ``shift`` where that sum is
    exact in bf16 (the base is a multiple of 2^-4 below 4, the shift a multiple of 2^-4 below 2)"""

    def __init__(self):
        g = torch.Generator().manual_seed(9)
        self.shift = (torch.randint(-31, 32, (1, 4, 6, 10), generator=g).float() / 16.0).to(torch.bfloat16)
        self.seen = []

    def net(self, x, t, y):
        base = (torch.round(torch.tanh(x.float() + t.view(-1, 1, 1, 1)) * 48.0) / 16.0).to(torch.bfloat16)
        out = base + self.shift * y.view(-1, 1, 1, 1).to(torch.bfloat16)  # y = 1 on the cond rows, 0 on the uncond rows
        self.seen.append(out)
        return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_constant_difference_reuse_stage_equals_the_float64_restatement(dtype):
    z, _ = _state(dtype)
    y = torch.tensor([1.0, 1.0, 0.0, 0.0])
    model = Shifted()
    tgrid = ODE(4, "euler", 4).t
    table, flags = [4.0, 2.5, 7.5], [0, 1, 1]
    deltas = []
    traj = G.sample_cfg_reuse(model, z, tgrid, table, flags, "euler", y=y, deltas=deltas)
    assert len(model.seen) == 3 and len(deltas) == 1 and model.seen[0].shape[0] == 4 and model.seen[1].shape[0] == 2
    d = deltas[0]
    assert torch.equal(d, model.shift[:, :3].expand(2, -1, -1, -1))  # c - u is the shift, exactly
    # each reuse stage's slope, recovered from the euler states, is R(R(c' - d) + R(w d)) of ITS cond rows - and because c' - d is exactly the
    # uncond rows' output here, also the refresh chain R(u + R(w d)) at that scale
    t32 = tgrid.float()
    y_state = z
    for i, (w, again) in enumerate(zip(table, flags)):
        out = model.seen[i]
        c = X.f64(out[:2, :3])
        if again:
            want = X.reuse_chain(c, X.f64(d), w)
            u = c - X.f64(d)
            assert np.array_equal(X.bf16_round64(u), u)
            g2, _ = X.refresh_chain(c, u, w)
            assert np.array_equal(want, g2)
        else:
            want, d64 = X.refresh_chain(c, X.f64(out[2:, :3]), w)
            assert X.same_bits(d, d64)
        slope = torch.cat([torch.cat([torch.from_numpy(want).to(torch.bfloat16)] * 2), torch.cat([out[:2, 3:]] * 2) if again else out[:, 3:]], 1)
        dt = t32[i + 1] - t32[i]
        y_state = y_state + dt * slope.to(dtype)
        assert torch.equal(traj[i + 1], y_state), (dtype, i)


@pytest.mark.parametrize("w", [1.5, 2.5, 4.5, -1.0, 0.0, 7.5])
def test_reuse_chain_on_bf16_ties_equals_the_float64_restatement(w):
    c2, d = X.midpoint_operands(w)
    # the operands do meet ties: the exact product / sum lies half way between two bf16 values for some elements
    prod = np.float64(np.float32(w)) * X.f64(d)
    ties = lambda v: int((np.abs(v - X.bf16_round64(v)) == np.abs(np.ldexp(1.0, np.frexp(v)[1] - 9))).sum())  # noqa: E731  (half an ulp)
    if w in (1.5, 2.5, 4.5):
        assert ties(prod[prod != 0]) >= 8  # (of 128 elements)
        s = X.bf16_round64(X.f64(c2) - X.f64(d)) + X.prod_bf16(w, X.f64(d))
        assert ties(s[s != 0]) >= 8

    class One:
        cfg_channels = 1

        def forward(self, x, t, y):
            return x.to(torch.bfloat16).to(x.dtype)

    x_cond = c2.view(1, 1, 8, 16)
    held = d.view(1, 1, 8, 16)
    class Pair(One):
        def forward(self, x, t, y):  # a refresh stage stores d: the cond row passes, the uncond row is 0; a reuse stage passes c'
            o = x.to(torch.bfloat16)
            return torch.cat([o[:1], torch.zeros_like(o[:1])]) if o.shape[0] == 2 else o

    # one refresh stage, then one reuse stage on c', straight through the evaluation the loops share
    func, call = G._reuse_func(Pair(), 2, [float(np.float32(w))] * 2, [0, 1], {"y": torch.zeros(2)}, {"y": torch.zeros(1)}, "cpu")
    g0 = func(torch.tensor(0.0), torch.cat([held, held]))
    want0, d64 = X.refresh_chain(X.f64(held), np.zeros((1, 1, 8, 16)), w)
    assert X.same_bits(g0[:1], want0) and X.same_bits(g0[1:], want0) and np.array_equal(d64, X.f64(held))
    g1 = func(torch.tensor(0.0), torch.cat([x_cond, x_cond]))
    want1 = X.reuse_chain(X.f64(x_cond), X.f64(held), w)
    assert call[0] == 2 and g1.dtype == torch.bfloat16
    assert X.same_bits(g1[:1], want1) and X.same_bits(g1[1:], want1), w


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_python_layer_refusals():
    z, y = _state(torch.bfloat16)
    tgrid = ODE(5, "euler", 4).t
    fours = [4.0] * 4
    with pytest.raises(ValueError, match="evaluation 0 reuses"):
        G.sample_cfg_reuse(Toy(), z, tgrid, fours, [1, 0, 1, 0], "euler", y=y)
    with pytest.raises(ValueError, match="rescale / norm_limit"):
        G.sample_cfg_reuse(Toy(), z, tgrid, fours, [0, 1, 0, 1], "euler", y=y, rescale=0.5)
    with pytest.raises(ValueError, match="rescale / norm_limit"):
        ODE(5, "euler", 4).sample(z, Toy().forward_with_cfg, cfg_table=fours, cfg_reuse=[0, 1, 0, 1], cfg_norm_limit=1.5, y=y)
    with pytest.raises(ValueError, match="packed batch"):
        G.sample_cfg_reuse(Toy(), [z[:1], z[:1]], tgrid, fours, [0, 1, 0, 1], "euler", y=y)
    with pytest.raises(ValueError, match="packed batch"):
        ODE(5, "euler", 4).sample([z[:1], z[:1]], Toy().forward_with_cfg, cfg_table=fours, cfg_reuse=[0, 1, 0, 1], y=y)
    with pytest.raises(ValueError, match="even batch"):
        G.sample_cfg_reuse(Toy(), z[:3], tgrid, fours, [0, 1, 0, 1], "euler", y=y[:3])
    with pytest.raises(ValueError, match="fixed-grid"):
        G.sample_cfg_reuse(Toy(), z, tgrid, fours, [0, 1, 0, 1], "abm2", y=y)
    with pytest.raises(ValueError, match="unknown multistep"):
        G.sample_cfg_reuse_multistep(Toy(), z, tgrid, fours, [0, 1, 0, 1], "euler", y=y)
    # rule parameters at their defaults are no rule
    got = G.sample_cfg_reuse(Toy(), z, tgrid, fours, [0, 1, 0, 1], "euler", y=y, rescale=0.0, norm_limit=float("inf"))
    assert torch.equal(got, G.sample_cfg_reuse(Toy(), z, tgrid, fours, [0, 1, 0, 1], "euler", y=y))


def test_sample_driver_flags():
    from lumina_t2x_amd import sample as S
    p = S.build_parser()
    base = ["--ckpt", "x", "--sampling-method", "midpoint"]
    tgrid = ODE(5, "midpoint", 4).t
    assert S.guidance_reuse(p.parse_args(base), tgrid, None) is None  # the default: the call it was
    assert S.guidance_reuse(p.parse_args(base + ["--cfg_reuse", "2"]), tgrid, None).tolist() == [0, 1] * 4
    assert S.guidance_reuse(p.parse_args(base + ["--cfg_reuse", "3"]), tgrid, None).tolist() == [0, 1, 1, 0, 1, 1, 0, 1]
    assert S.guidance_reuse(p.parse_args(base + ["--cfg_reuse_per_step"]), tgrid, None).tolist() == [0, 1] * 4
    args = p.parse_args(base + ["--cfg_reuse", "2", "--cfg_interval", "0.1", "0.8"])
    table = S.guidance_table(args, tgrid)
    flags = S.guidance_reuse(args, tgrid, table)
    assert bool((flags[table == 1] == 0).all()) and int(flags.sum()) == int((table != 1).sum()) // 2
    for extra in (["--cfg_rescale", "0.5"], ["--cfg_norm_limit", "1.5"]):
        with pytest.raises(SystemExit, match="cfg_rescale"):
            S.guidance_reuse(p.parse_args(base + ["--cfg_reuse", "2"] + extra), tgrid, None)
    with pytest.raises(SystemExit, match="K >= 2"):
        S.guidance_reuse(p.parse_args(base + ["--cfg_reuse", "1"]), tgrid, None)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_documented():
    declared = set(_lib.declared_symbols())
    text = _lib.header_text(strip_comments=False)
    for name in NEW:
        assert name in declared and name in _lib._SIGNATURES, name
    for word in ("reuse_host", "DESIGN.md 7k", "R(R(c' - d) + R(w d))", "three HIP-graph keys"):
        assert word in text, word
