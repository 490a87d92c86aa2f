"""Composed guidance on the CPU: ``transport.guidance.guided_compose`` / ``compose_table`` / ``sample_cfg_compose`` - the definition the
engine calls are held to (tests/test_gpu_compose.py).

* exactness: on operands that keep every intermediate exact the chain equals its float64 restatement word for word;
* at K = 1 it is ``uncond + w * (cond - uncond)`` evaluated by torch in bf16;
* three mutants of the chain each move at least one word;
* the weight table: shapes, intervals, stage counts; a prompt of weight 0 is the K - 1 composition;
* the Python refusals, by name."""
import math

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.integrators import fixed_grid_odeint
from lumina_t2x_amd.transport.mini import ODE

import exact_compose as X


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("Bp", [1, 2])
@pytest.mark.parametrize("K", [1, 2, 3, 7])
def test_chain_equals_its_float64_restatement_on_exact_operands(K, Bp, ch, dtype):
    outs, w = X.exact_outs(K, Bp, 4, 6, 10, dtype, seed=K * 10 + Bp)
    got = G.guided_compose(outs, w, ch)
    want = X.compose64(outs, w, ch, exact=True)
    assert got.dtype == dtype and tuple(got.shape) == (Bp, 4, 6, 10)
    assert torch.equal(X.words(got), X.words(want))
    assert torch.equal(X.words(got[:, ch:]), X.words(outs[:Bp, ch:]))  # past cfg_channels: prompt 1's rows, copied
    assert len(torch.unique(got[:, :ch].float())) > 8  # (the operands exercise the chain)


@pytest.mark.parametrize("w", [4.0, 1.0, -0.75, 2.3])
def test_one_prompt_is_classifier_free_guidance_in_bf16(w):
    outs, _ = X.random_outs(1, 2, 4, 8, 8, torch.bfloat16, seed=3)
    cond, uncond = outs[:2], outs[2:]
    want = torch.cat([uncond[:, :3] + w * (cond[:, :3] - uncond[:, :3]), cond[:, 3:]], 1)
    assert want.dtype == torch.bfloat16
    assert torch.equal(X.words(G.guided_compose(outs, [w], 3)), X.words(want))
    # an fp32 state holds the same bf16 values: R is bf16 whatever the dtype
    assert torch.equal(G.guided_compose(outs.float(), [w], 3), want.float())


def test_three_mutants_each_move_a_word():
    """stated input: K = 3, B' = 2, random bf16 outputs of scale 3 (seed 5) and the weights drawn with them"""
    outs, w = X.random_outs(3, 2, 4, 8, 8, torch.bfloat16, seed=5)
    good = G.guided_compose(outs, w, 3)
    assert torch.equal(X.words(X.compose_stated(outs, w, 3)), X.words(good))  # the restatement the mutants are cut from is the chain
    for mutant in ("reverse", "drop_inner", "base_from_last"):
        moved = int((X.words(X.compose_stated(outs, w, 3, **{mutant: True})) != X.words(good)).sum())
        assert moved >= 1, mutant
    # the mutants leave the copied channels alone
    assert torch.equal(X.compose_stated(outs, w, 3, reverse=True)[:, 3:], good[:, 3:])


def test_compose_table_shapes_intervals_and_stage_counts():
    tgrid = torch.linspace(0.0, 1.0, 5)
    for method, stages in (("euler", 1), ("midpoint", 2), ("rk4", 4)):
        tab = G.compose_table(tgrid, method, [2.0, -1.0, 0.5])
        assert tab.dtype == torch.float32 and tuple(tab.shape) == (4 * stages, 3)
        assert torch.equal(tab, torch.tensor([2.0, -1.0, 0.5]).repeat(4 * stages, 1))
        ts = G.stage_times(tgrid, method, torch.float32, False)
        tab = G.compose_table(tgrid, method, [2.0, -1.0, 0.5], [None, (0.25, 0.75), (0.0, 0.0)])
        inside = (ts >= 0.25) & (ts < 0.75)
        assert torch.equal(tab[:, 0], torch.full((4 * stages,), 2.0))
        assert torch.equal(tab[:, 1], torch.where(inside, torch.tensor(-1.0), torch.tensor(0.0)))
        assert torch.equal(tab[:, 2], torch.zeros(4 * stages)) and 0 < int(inside.sum()) < 4 * stages
        # the time test is cfg_table's
        assert torch.equal(tab[:, 1] != 0, G.cfg_table(tgrid, method, 5.0, interval=(0.25, 0.75)) != 1)
    with pytest.raises(ValueError, match="fixed-grid methods"):
        G.compose_table(tgrid, "ab2", [1.0])
    with pytest.raises(ValueError, match="2 intervals for K = 3"):
        G.compose_table(tgrid, "euler", [1.0, 1.0, 1.0], [None, None])
    with pytest.raises(ValueError, match="empty or not ordered"):
        G.compose_table(tgrid, "euler", [1.0], [(0.8, 0.2)])


@pytest.mark.parametrize("j", [0, 1, 2])
def test_a_prompt_of_weight_zero_is_the_composition_without_it(j):
    outs, w = X.random_outs(3, 2, 4, 8, 8, torch.bfloat16, seed=7)
    w[j] = 0.0
    rows = list(outs.chunk(4))
    less = torch.cat(rows[:j] + rows[j + 1:])
    got, want = G.guided_compose(outs, w, 3), G.guided_compose(less, w[:j] + w[j + 1:], 3)
    assert torch.equal(X.words(got[:, :3], fold_zero=True), X.words(want[:, :3], fold_zero=True))
    if j:  # (the copied channels are prompt 1's)
        assert torch.equal(got[:, 3:], want[:, 3:])


def _toy(x, t, y):
    """a model whose output depends on its row's label and time: out = (x + y) * t, in the state dtype"""
    return ((x.float() + y[:, None, None, None].float()) * t[:, None, None, None]).to(torch.bfloat16).to(x.dtype)


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_host_loop_is_fixed_grid_odeint_around_the_composed_velocity(method):
    K, Bp = 2, 2
    z = torch.randn(Bp, 4, 4, 6, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    y = torch.tensor([1.0, 2.0, -1.0, 0.5, 0.0, 0.0])
    tgrid = ODE(4, method, 4).t
    table = G.compose_table(tgrid, method, [2.0, -0.5], [None, (0.0, 0.6)])
    table[1, 0] = 3.0  # (a table that varies per stage)
    got = G.sample_cfg_compose(_toy, z, tgrid, table, K, method, y=y)
    calls = []

    def vel(tt, s):
        calls.append(float(tt))
        tv = torch.ones(6) * tt
        return G.guided_compose(_toy(s.repeat(3, 1, 1, 1), tv, y), table[len(calls) - 1].tolist(), 3)

    want = fixed_grid_odeint(vel, z, tgrid, method=method)
    assert tuple(got.shape) == (4, Bp, 4, 4, 6) and torch.equal(X.words(got), X.words(want))
    assert len(calls) == table.shape[0]
    assert torch.equal(ODE(4, method, 4).sample(z, _toy, compose=table, y=y), got)


def test_python_refusals_by_name():
    z = torch.zeros(1, 4, 4, 4)
    y = torch.zeros(3)
    tgrid = [0.0, 0.5, 1.0]
    tab = G.compose_table(tgrid, "euler", [1.0, 1.0])
    with pytest.raises(ValueError, match=r"K = 8 prompts \(1 \.\. 7\)"):
        G.check_compose([1.0] * 8)
    with pytest.raises(ValueError, match="not finite"):
        G.check_compose([1.0, math.inf])
    with pytest.raises(ValueError, match="not finite"):
        G.guided_compose(torch.zeros(3, 4, 2, 2), [1.0, math.nan])
    with pytest.raises(ValueError, match=r"4 rows are not a multiple of K \+ 1 = 3"):
        G.guided_compose(torch.zeros(4, 4, 2, 2), [1.0, 1.0])
    for ch in (0, 5):
        with pytest.raises(ValueError, match=rf"cfg_channels {ch} outside 1\.\.4"):
            G.guided_compose(torch.zeros(3, 4, 2, 2), [1.0, 1.0], ch)
    with pytest.raises(ValueError, match="the weight table has 2 rows, the grid has 4 stages"):
        G.sample_cfg_compose(_toy, z, tgrid, tab, 2, "midpoint", y=y)
    with pytest.raises(ValueError, match=r"the weights are for 2 prompts, the call has K = 3"):
        G.sample_cfg_compose(_toy, z, tgrid, tab, 3, "euler", y=y)
    with pytest.raises(ValueError, match=r"conditioning 'y' has 2 rows.*\(K \+ 1\) B' = 3 rows"):
        G.sample_cfg_compose(_toy, z, tgrid, tab, 2, "euler", y=y[:2])
    # the front end: what composed guidance is not served with, by name
    o = ODE(3, "euler", 4)
    tab = G.compose_table(o.t, "euler", [1.0, 1.0])
    for kw, needle in ((dict(cfg_table=torch.ones(2)), r"guidance table \(cfg_table\)"), (dict(cfg_rescale=0.5), "rescale / norm limit"),
                       (dict(cfg_norm_limit=2.0), "rescale / norm limit"), (dict(cfg_reuse=torch.zeros(2)), r"guidance reuse"),
                       (dict(slg_table=torch.ones(2)), "skip-layer guidance"), (dict(pag_table=torch.ones(2)), "perturbed-attention guidance"),
                       (dict(cfg_apg=dict(eta=0.0)), "projected guidance"), (dict(cfg_zero_star=True), "projected guidance"),
                       (dict(teacache=0.1), "step caching"), (dict(mask=torch.ones(4, 4)), "inpainting mask"),
                       (dict(windows=([(0, 0)], (4, 4))), r"tiled sampling \(windows\)")):
        with pytest.raises(NotImplementedError, match=rf"composed guidance \(compose\) and .*{needle}.* are not served together"):
            o.sample(z, _toy, compose=tab, y=y, **kw)
    with pytest.raises(NotImplementedError, match="packed batch"):
        o.sample([z[0]], _toy, compose=tab, y=y)
    for method in ("ab2", "abm3", "dopri5"):
        with pytest.raises(NotImplementedError, match=rf"fixed-grid methods euler, midpoint, rk4, not '{method}'.*multistep and adaptive"):
            ODE(3, method, 4).sample(z, _toy, compose=tab, y=y)
    assert _lib.LT_COMPOSE_MAX == G.COMPOSE_MAX == 7


def test_driver_arguments_build_the_table():
    from lumina_t2x_amd import sample as S
    base = ["--ckpt", "x", "--caption_path", "y", "--image_save_path", "z", "--sampling-method", "midpoint"]
    tgrid = ODE(5, "midpoint", 4).t
    assert S.compose_plan(S.build_parser().parse_args(base), tgrid) is None  # the defaults make the call they made
    args = S.build_parser().parse_args(base + ["--compose_prompts", "a cat", "a hat", "--compose_weights", "4", "-1.5",
                                               "--compose_interval", "2", "0.0", "0.5"])
    prompts, table = S.compose_plan(args, tgrid)
    assert prompts == ["a cat", "a hat"]
    assert torch.equal(table, G.compose_table(tgrid, "midpoint", [4.0, -1.5], [None, (0.0, 0.5)]))
    for extra, needle in ((["--compose_weights", "1"], "belong to --compose_prompts"),
                          (["--compose_prompts", "a", "b", "--compose_weights", "1"], "needs as many weights"),
                          (["--compose_prompts", "a", "--compose_weights", "1", "--compose_interval", "2", "0", "1"], "counted from 1 to 1"),
                          (["--compose_prompts"] + ["p"] * 8 + ["--compose_weights"] + ["1"] * 8, "at most 7")):
        with pytest.raises(SystemExit, match=needle):
            S.compose_plan(S.build_parser().parse_args(base + extra), tgrid)
