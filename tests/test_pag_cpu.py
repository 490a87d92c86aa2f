"""CPU: perturbed-attention guidance - the tables, the refusals, the host loop on a stub model, and the operator chain of a
perturbed evaluation in float64 (tests/pag_chain.py on tests/forward_chain.py, imported unchanged).

Bounds.  The float64 chain projects V alone where the restatement slices the Q | K | V projection, so the two differ by float64 summation
order only: EQUAL = 1e-10 relative (float64 eps 1.1e-16 times a few thousand operations per word; seven orders below the gate).  A change of
meaning must move the output by more than GATE, the CPU chain test's own gate (tests/test_forward_chain_cpu.py)."""
import dataclasses
import math

import pytest
import torch

from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE

import forward_chain as FC
import pag_chain as PC
from test_forward_chain_cpu import GATE

EQUAL = 1e-10
DEPTH = 4
CHAIN_GOLDENS = ("nextdit_tiny", "nextdit_tiny_gqa", "imagenet_tiny", "flag_tiny", "moe_tiny")


def deep_case(golden_dir, name, depth=DEPTH):
    """the golden's plain forward on a model of `depth` blocks (the golden's config and seed, as tests/test_gpu_slg.py deepens it)"""
    from oracle import synth
    c0 = FC.golden_case(golden_dir, name, "forward")
    cfg = dataclasses.replace(c0.cfg, n_layers=depth)
    g, _, _ = FC.load_golden(golden_dir, name)
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    i = c0.inputs
    kw = dict(use_cfg=False, scale_watershed=0.0, name=f"{name}-deep{depth}")
    if c0.fam["text"]:
        kw.update(cap=i["cap"], mask=i["mask"])
    else:
        kw.update(labels=i["labels"])
    return FC.Case(cfg, sd, i["x"], i["t"], **kw)


# ---- tables and refusals ------------------------------------------------------------------------------------------------------------------------
def test_pag_table_follows_the_slg_rule():
    tgrid = ODE(5, "midpoint", 4).t
    for interval in (None, (0.2, 0.7), (0.5, 0.5)):
        assert torch.equal(G.pag_table(tgrid, "midpoint", 2.5, interval), G.slg_table(tgrid, "midpoint", 2.5, interval))
    assert G.pag_table(tgrid, "midpoint", 2.5).tolist() == [2.5] * 8 and not G.pag_table(tgrid, "euler", 3.0, (0.5, 0.5)).any()
    with pytest.raises(ValueError, match="not ordered"):
        G.pag_table(tgrid, "euler", 1.0, (0.7, 0.2))
    with pytest.raises(ValueError, match="perturbed-attention table has an entry that is not finite"):
        G.pag_table(tgrid, "euler", math.inf)
    with pytest.raises(ValueError, match="perturbed-attention table has 3 entries"):
        G.check_pag([1.0, 2.0, 3.0], tgrid, "euler")
    with pytest.raises(ValueError, match="perturbed-attention table is None"):
        G.check_pag(None, tgrid, "euler")


def test_check_pag_layers():
    assert G.check_pag_layers([2, 0], [1], 4) == ([2, 0], [1])
    assert G.check_pag_layers(torch.tensor([0, 1, 2, 3]), (), 4) == ([0, 1, 2, 3], [])     # P may hold every layer
    assert G.check_pag_layers((), [1]) == ([], [1])
    for P, S, n, word in (([1.5], (), 4, "not an integer"), ([True], (), 4, "not an integer"), ([1, 1], (), 4, "perturb index 1 is repeated"),
                          ([4], (), 4, "perturb index 4 is outside 0..3"), ([-1], (), 4, "outside 0..3"), ([1, 2], [2], 4, "layer 2 is in the skip set and in"),
                          ([1], [0, 0], 4, "skip index 0 is repeated"), ([], [0, 1, 2, 3], 4, "leaves no layer")):
        with pytest.raises(ValueError, match=word):
            G.check_pag_layers(P, S, n)


def test_refuse_with_pag_names_every_companion():
    tab = torch.ones(4)
    G.refuse_with_pag(None, method="dopri5", rescale=0.5, slg=tab)      # no table: nothing to refuse
    G.refuse_with_pag(tab, method="rk4")
    for kw, word in ((dict(rescale=0.5), "rescale / norm_limit rule"), (dict(norm_limit=2.0), "rescale / norm_limit rule"),
                     (dict(reuse=[0, 1, 0, 1]), "guidance reuse"), (dict(method="abm2"), "not 'abm2'"), (dict(method="dopri5"), "not 'dopri5'"),
                     (dict(teacache=0.1), "step caching"), (dict(mask=torch.ones(1)), "inpainting mask"), (dict(slg=tab), "together with an slg table")):
        with pytest.raises(ValueError, match=word):
            G.refuse_with_pag(tab, **{"method": "euler", **kw})


class _Stub:
    """a model whose forward is cheap and depends on every argument: blocks scale the state, a skipped block is left out, a perturbed one
    contributes another factor"""
    n_layers, cfg_channels = 4, 3

    def __init__(self):
        self.calls = []

    def forward(self, x, t, y, skip_layers=(), perturb_layers=()):
        self.calls.append((tuple(skip_layers), tuple(perturb_layers), x.shape[0]))
        h = x.float()
        for l in range(self.n_layers):
            if l in skip_layers:
                continue
            h = h * (1.0 + 0.125 * (l + 1)) + (0.5 if l in perturb_layers else 0.25) * y.float().view(-1, 1, 1, 1) - 0.0625 * t.view(-1, 1, 1, 1)
        return h.to(x.dtype)

    def forward_with_cfg(self, x, t, y, cfg_scale):
        half = x.shape[0] // 2
        o = self.forward(torch.cat([x[:half]] * 2), t, y).to(torch.bfloat16)
        c, u = o[:half, :3], o[half:, :3]
        g = u + cfg_scale * (c - u)
        return torch.cat([torch.cat([g, o[:half, 3:]], 1), torch.cat([g, o[half:, 3:]], 1)]).to(x.dtype)


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_host_loop_identities_on_a_stub_model(method, dtype):
    stages = {"euler": 1, "midpoint": 2, "rk4": 4}[method]
    tgrid = ODE(4, method, 4).t
    n = 3 * stages
    w = torch.tensor(([4.0, 1.0, 3.0, 1.0, 2.5, 1.0] * 2)[:n])
    s = torch.tensor(([2.0, 0.0, 0.0, 1.5, -1.0, 3.0] * 2)[:n])
    z = torch.randn(1, 4, 4, 6, generator=torch.Generator().manual_seed(3)).to(dtype).repeat(2, 1, 1, 1)
    y = torch.tensor([1.0, -1.0])
    m = _Stub()
    # every s == 0: the schedule loop, bit for bit
    got = G.sample_cfg_pag(m, z, tgrid, w, torch.zeros(n), [1, 2], [3], method, y=y)
    assert torch.equal(got, G.sample_cfg_schedule(m, z, tgrid, w, method, y=y))
    # P empty: skip-layer guidance, bit for bit
    got = G.sample_cfg_pag(m, z, tgrid, w, s, [], [1, 2], method, y=y)
    assert torch.equal(got, G.sample_cfg_slg(m, z, tgrid, w, s, [1, 2], method, y=y))
    # P given: the third evaluation takes both sets, on the cond rows alone, and the result moves
    m.calls.clear()
    pag = G.sample_cfg_pag(m, z, tgrid, w, s, [2, 0], [3], method, y=y)
    third = [c for c in m.calls if c[0] or c[1]]
    assert third == [((3,), (2, 0), 1)] * int((s != 0).sum())
    assert not torch.equal(pag, got)
    for bad, word in ((dict(pag_layers=[1], skip_layers=[1]), "disjoint"), (dict(pag_layers=[], skip_layers=[]), "both layer sets are empty"),
                      (dict(pag_layers=[4]), "outside 0..3"), (dict(pag_layers=[1], rescale=0.5), "rescale"), (dict(pag_layers=[1], reuse=[0] * n), "reuse")):
        kw = dict(pag_layers=bad.pop("pag_layers"), skip_layers=bad.pop("skip_layers", ()))
        with pytest.raises(ValueError, match=word):
            G.sample_cfg_pag(m, z, tgrid, w, s, kw["pag_layers"], kw["skip_layers"], method, y=y, **bad)
    with pytest.raises(ValueError, match="packed batch"):
        G.sample_cfg_pag(m, [z[0], z[1]], tgrid, w, s, [1], (), method, y=y)


def test_front_ends_refuse_by_name():
    m = _Stub()
    z = torch.zeros(2, 4, 4, 6)
    y = torch.tensor([1.0, -1.0])
    tab = torch.ones(3)
    o = ODE(4, "euler", 4)
    for kw, exc, word in ((dict(slg_table=tab), ValueError, "together with an slg table"), (dict(cfg_rescale=0.5), ValueError, "rescale"),
                          (dict(cfg_reuse=[0, 1, 1]), ValueError, "guidance reuse"), (dict(teacache=0.1), ValueError, "step caching"),
                          (dict(mask=torch.ones(1, 1, 4, 6)), ValueError, "inpainting mask")):
        with pytest.raises(exc, match=word):
            o.sample(z, m.forward_with_cfg, cfg_table=tab * 4, pag_table=tab, pag_layers=[1], y=y, **kw)
    with pytest.raises(ValueError, match="packed batch"):
        o.sample([z[0], z[1]], m.forward_with_cfg, cfg_table=tab * 4, pag_table=tab, pag_layers=[1], y=y)
    with pytest.raises(ValueError, match="not 'abm2'"):
        ODE(4, "abm2", 4).sample(z, m.forward_with_cfg, cfg_table=tab * 4, pag_table=tab, pag_layers=[1], y=y)
    got = o.sample(z + 1, m.forward_with_cfg, cfg_table=tab * 4, pag_table=tab, pag_layers=[1], slg_layers=[2], y=y)
    assert torch.equal(got, G.sample_cfg_pag(m, z + 1, o.t, tab * 4, tab, [1], [2], "euler", y=y))


# ---- the operator chain ---------------------------------------------------------------------------------------------------------------------------
_CHAIN = {}


def chain(golden_dir, name):
    """(case, paths, unperturbed steps, unperturbed float64 output), computed once per golden"""
    if name not in _CHAIN:
        case = deep_case(golden_dir, name)
        paths = {}
        steps = FC.build(case, paths)
        _CHAIN[name] = (case, paths, steps, FC.run(PC.Torch64(case), steps))
    return _CHAIN[name]


@pytest.mark.parametrize("name", CHAIN_GOLDENS)
def test_perturbed_chain_equals_the_identity_matrix_restatement(golden_dir, name):
    case, _, steps, base = chain(golden_dir, name)
    for P, S in (((1,), ()), ((0, 1, 2, 3), ()), ((1,), (2,)), ((3,), (0,))):
        got = FC.run(PC.Torch64(case), PC.pag_steps(case, steps, P, S))
        eye = PC.EyeTorch64(case, P)
        want = FC.run(eye, PC.pag_steps(case, steps, (), S), eye.hook)
        err, moved = FC.rel_l2(got, want), FC.rel_l2(got, base)
        print(f"{case.name} P={P} S={S}: rel_l2 to the restatement {err:.3e}, to the unperturbed chain {moved:.3e}")
        assert err < EQUAL, (case.name, P, S, err)
        assert moved > GATE, (case.name, P, S, moved, GATE)


@pytest.mark.parametrize("name", CHAIN_GOLDENS)
def test_every_pag_mutation_moves_the_float64_chain_past_the_gate(golden_dir, name):
    case, _, steps, _ = chain(golden_dir, name)
    P = (1, 3)
    psteps = PC.pag_steps(case, steps, P)
    base = FC.run(PC.Torch64(case), psteps)
    gqa = case.cfg.kv_heads != case.cfg.n_heads
    muts = PC.pag_mutations(case, psteps, P)
    assert len(muts) == len(P) * (5 if case.fam["text"] else 2)
    for mname, hook, gqa_only in muts:
        moved = FC.rel_l2(FC.run(PC.Torch64(case), psteps, hook), base)
        print(f"{case.name} {mname}: {moved:.3e}")
        if gqa_only and not gqa:
            assert moved == 0.0, (case.name, mname, moved)     # with H == Hkv both head maps are the identity
        else:
            assert moved > GATE, (case.name, mname, moved, GATE)


def test_the_gqa_fixture_sees_the_head_map(golden_dir):
    case, _, _, _ = chain(golden_dir, "nextdit_tiny_gqa")
    H, Hkv = case.cfg.n_heads, case.cfg.kv_heads
    assert Hkv < H and PC.head_index(H, Hkv, "div") != PC.head_index(H, Hkv, "mod")
