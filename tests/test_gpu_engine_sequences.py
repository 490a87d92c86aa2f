"""GPU: one long-lived engine taking different calls one after another (the catalogue, driver and circuit are tests/engine_sequences.py).

The expected value of an entry is its result on a FRESH model of the same state dict with the engine option ``graph`` at 0, the entry's settings
applied and that call alone run: the project's own path, verified per feature elsewhere, with nothing in it that could see state another
call left behind.  An entry that legitimately reads what an earlier call stored (``forward_with_cfg_reuse(reuse=True)``,
``forward_cached(..., "reuse")``) is expected to be refused by name, or to equal the fresh run of the storing entry followed by it - which of
the two follows from the documented contract (engine_sequences' module docstring), not from the engine.  Everything is compared bit for bit;
there is no tolerance in this file."""
import contextlib
import functools
import time

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.engine import DiTEngine, EngineLimits
from oracle import synth

import engine_sequences as ES
from test_gpu_slg import _build, _deep

pytestmark = pytest.mark.gpu

LIMITS = EngineLimits(max_batch=4, max_tokens=4096, max_text=256)  # room for every entry: no call replaces the engine
_REF, _INPUTS = {}, {}


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _inputs(golden_dir, family):
    if family not in _INPUTS:
        _INPUTS[family] = ES.Inputs(family, _deep(golden_dir, family)[2])
    return _INPUTS[family]


def _fresh(golden_dir, family, seed=None):
    cfg, sd, _ = _deep(golden_dir, family)
    if seed is not None:
        sd = synth.synth_state_dict(cfg, seed=seed)
    model = _build(family, cfg, sd)
    model.engine_limits = LIMITS
    return model


def _keep(out):
    if isinstance(out, ES.Refused):
        return out
    return tuple(t.clone() for t in out[0]), tuple(int(v) for v in out[1])


@contextlib.contextmanager
def _counted(model, names):
    """counts the calls of the named methods of the model's class and of the engine class while the block runs"""
    calls, saved = {n: 0 for n in names}, []
    for cls in (type(model), DiTEngine):
        for n in names:
            if n not in cls.__dict__ and not any(n in b.__dict__ for b in cls.__mro__[1:]):
                continue
            orig = getattr(cls, n)

            def wrapper(*a, _orig=orig, _n=n, **k):
                calls[_n] += 1
                return _orig(*a, **k)
            had = n in cls.__dict__
            setattr(cls, n, functools.wraps(orig)(wrapper))
            saved.append((cls, n, orig, had))
    try:
        yield calls
    finally:
        for cls, n, orig, had in reversed(saved):
            if had:
                setattr(cls, n, orig)
            else:
                delattr(cls, n)


def _reference(golden_dir, family, chain, options=(), seed=None):
    """the last entry of ``chain`` (the entry alone, or the entry that stored what it reads and then the entry) on a fresh model, graph 0"""
    key = (family, seed, tuple(options), tuple(e.name for e in chain))
    if key not in _REF:
        model = _fresh(golden_dir, family, seed)
        drv = ES.Driver(model, _inputs(golden_dir, family), base_options=tuple(options) + (("graph", 0),))
        for e in chain:
            with _counted(model, e.methods) as calls:
                out = drv.run(e)
            assert not isinstance(out, ES.Refused), (key, out.message)
            assert all(calls.values()), (e.name, calls)  # the entry goes through every method it names
        assert model._engine.graph_replays() == 0
        _REF[key] = _keep(out)
        for t in _REF[key][0]:
            assert bool(torch.isfinite(t.float()).all()), key
        del drv, model
    return _REF[key]


def _differing(got, want):
    """words and counters that differ (None: not comparable)"""
    if len(got[0]) != len(want[0]) or len(got[1]) != len(want[1]):
        return None
    n = sum(a != b for a, b in zip(got[1], want[1]))
    for a, b in zip(got[0], want[0]):
        if a.shape != b.shape or a.dtype != b.dtype:
            return None
        if not torch.equal(_bits(a), _bits(b)):
            n += int((_bits(a) != _bits(b)).sum())
    return n


def _visit(golden_dir, family, drv, entry, options=(), seed=None, record=None):
    """run one entry on the long-lived engine and compare it with what the contract expects: None, or the words of what went wrong;
    ``record``: a list that takes what the visit returned"""
    drv.apply(entry)
    exp = drv.expectation(entry)
    got = drv.run(entry)
    if record is not None:
        record.append(_keep(got))
    if exp is not None and exp[0] == "refused":
        if not isinstance(got, ES.Refused):
            return f"served, but the contract refuses it ({exp[1]})"
        return None if all(w in got.message for w in exp[1]) else f"refused without naming the cause {exp[1]}: {got.message}"
    if isinstance(got, ES.Refused):
        return f"refused: {got.message}"
    chain = [entry] if exp is None else [exp[1], entry]
    diff = _differing(got, _reference(golden_dir, family, chain, options, seed))
    return None if diff == 0 else ("outputs of another form" if diff is None else f"{diff} words differ")


def _walk(golden_dir, family, drv, cat, walk, options=(), seed=None, seen=None, limit=8, record=None):
    """visit cat[i] for i in walk; the failures as report lines (at most ``limit``, then the walk ends)"""
    eng, seen, lines = drv.eng, {} if seen is None else seen, []
    prev = None
    for n, i in enumerate(walk):
        e = cat[i]
        r0 = eng.graph_replays()
        bad = _visit(golden_dir, family, drv, e, options, seed, record)
        s = seen.setdefault(e.name, dict(passed=0, eager=0, replayed=0))
        if e.keys:
            s["replayed" if eng.graph_replays() > r0 else "eager"] += 1
        if bad is None:
            s["passed"] += 1
        else:
            lines.append(f"visit {n}: {prev} -> {e.name}: {bad}; the entry passed {s['passed']} time(s) earlier in the walk")
            if len(lines) >= limit:
                break
        prev = e.name
    return lines


# ---- 1. every ordered pair -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(ES.CATALOGUES))
def test_every_ordered_pair_on_one_engine(golden_dir, family):
    cat = ES.CATALOGUES[family]
    for e in cat:  # (the references first, so that the walk's time is the walk's)
        if e.needs is None:
            _reference(golden_dir, family, [e])
    drv = ES.Driver(_fresh(golden_dir, family), _inputs(golden_dir, family))
    walk = ES.circuit(len(cat))
    assert len(walk) == len(cat) ** 2 + 1
    before, seen, t0 = drv.eng.graph_replays(), {}, time.perf_counter()
    lines = _walk(golden_dir, family, drv, cat, walk, seen=seen)
    print(f"{family}: {len(walk)} visits in {time.perf_counter() - t0:.1f} s, {drv.eng.graph_replays() - before} replays")
    assert not lines, "\n".join(lines)
    assert drv.eng.graph_replays() > before
    assert any(s["eager"] and s["replayed"] for s in seen.values())
    if family == "next":
        assert ES.distinct_keys(cat) > 16  # more keys than the cache holds: the walk evicts and re-captures


# ---- 2. the bound of the graph cache ------------------------------------------------------------------------------------------------------------
def test_graph_cache_bound(golden_dir):
    model = _fresh(golden_dir, "next")
    I = _inputs(golden_dir, "next")
    lim, p = model.engine_limits, model.patch_size
    shapes = [(16 * p, (33 + k) * p) for k in range(18)]  # 16 x (33 + k) tokens, two rows each
    assert all(h % p == 0 and w % p == 0 and 1024 < 2 * (h // p) * (w // p) and (h // p) * (w // p) <= lim.max_tokens for h, w in shapes)
    zs = [ES.hashed((1, 4, h, w), 50 + w).repeat(2, 1, 1, 1).to("cuda", torch.bfloat16) for h, w in shapes]
    want = []
    for z in zs:
        ref = _fresh(golden_dir, "next")
        ES.Driver(ref, I, base_options=(("graph", 0),))
        want.append(ref.forward_with_cfg(z, I.t, **I.kw()).clone())
        assert ref._engine.graph_replays() == 0
        del ref
    drv = ES.Driver(model, I)
    used = []
    for phase, order in enumerate((list(range(16)) * 3, list(range(18)) * 3, list(range(16)))):
        before, start = drv.eng.graph_replays(), len(used)
        for k in order:
            got = model.forward_with_cfg(zs[k], I.t, **I.kw())
            assert torch.equal(_bits(got), _bits(want[k])), (phase, k, int((got != want[k]).sum()))
            used.append(k)
        # the rule in forward_graphed_body: first use eager, later uses replay, a 17th key drops the oldest, a dropped key starts over
        assert drv.eng.graph_replays() - before == ES.fifo_replays(used) - ES.fifo_replays(used[:start]), phase
    # 16 held keys replay on their second and third lap; of the 18, the 16 still held replay once and every later use is a first use
    assert ES.fifo_replays(used[:48]) == 32 and ES.fifo_replays(used[:102]) == 48 and ES.fifo_replays(used) == 48


# ---- 3. two engines ------------------------------------------------------------------------------------------------------------------------------
def _pick(family, names):
    by = {e.name: e for e in ES.CATALOGUES[family]}
    return [by[n] for n in names]


def test_two_engines_interleaved(golden_dir):
    cat = _pick("next", ["cfg_bf16@48", "forward@16", "cfg_reuse_store@48", "cfg_reuse_use@48", "teacache_huge@16", "slg_traj@48", "packed_cfg_large",
                         "views@16"])
    seeds = (None, 12345)
    I = _inputs(golden_dir, "next")
    drvs = [ES.Driver(_fresh(golden_dir, "next", s), I) for s in seeds]
    a, b = _reference(golden_dir, "next", [cat[0]], seed=seeds[0]), _reference(golden_dir, "next", [cat[0]], seed=seeds[1])
    assert _differing(a, b) != 0  # two models
    walk = ES.circuit(len(cat))
    half = len(walk) // 2
    lines = []
    for n in range(len(walk) - 1):
        for who, i in ((0, walk[n]), (1, walk[(n + half) % (len(walk) - 1)])):
            bad = _visit(golden_dir, "next", drvs[who], cat[i], seed=seeds[who])
            if bad is not None:
                lines.append(f"step {n}, engine {who}: {cat[i].name}: {bad}")
        assert len(lines) < 8, "\n".join(lines)
    assert not lines, "\n".join(lines)
    assert all(d.eng.graph_replays() > 0 for d in drvs)


# ---- 4. options between calls -----------------------------------------------------------------------------------------------------------------
def test_option_changes_between_calls(golden_dir):
    cat = _pick("next", ["cfg_bf16@48", "forward@16", "ode_midpoint@48", "cfg_reuse_store@16", "cfg_reuse_use@16", "teacache_huge@48"])
    drv = ES.Driver(_fresh(golden_dir, "next"), _inputs(golden_dir, "next"))
    walk = ES.circuit(len(cat))
    pair = drv.eng.get_option("pair_layout")
    laps = []
    for options in ((("attention_variant", 3),), (("attention_variant", 4),), (("pair_layout", 1 - pair),), (("graph", 0),), ()):
        drv.set_base_options(options)
        for lap in range(3):
            laps.append([])
            lines = _walk(golden_dir, "next", drv, cat, walk, options=options, record=laps[-1])
            assert not lines, f"{options}, lap {lap}:\n" + "\n".join(lines)
    # the last lap (nothing overridden any more) equals the first (attention_variant 3), visit for visit, bit for bit.  Where the contract
    # refuses a reuse in one of the two laps and serves it in the other there is nothing to compare: the first lap begins behind an option
    # change, which prepares the conditioning again, the last lap finds what the lap before it stored
    first, last = laps[0], laps[-1]
    assert drv.options == {} and len(laps) == 15 and len(first) == len(last) == len(walk)
    both = [(a, b) for a, b in zip(first, last) if not isinstance(a, ES.Refused) and not isinstance(b, ES.Refused)]
    one = [i for i, (a, b) in zip(walk, zip(first, last)) if isinstance(a, ES.Refused) != isinstance(b, ES.Refused)]
    assert all(cat[i].needs is not None for i in one) and len(both) >= len(walk) - len(cat)
    assert all(_differing(a, b) == 0 for a, b in both)


# ---- 5. refused calls ---------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_sequence_intact(golden_dir):
    cat = _pick("next", ["cfg_bf16@48", "forward@16", "cfg_schedule@48", "teacache_0@16"])
    I = _inputs(golden_dir, "next")
    model = _fresh(golden_dir, "next")
    drv = ES.Driver(model, I)
    eng, z, t, g3 = drv.eng, I.z[16], I.t, ES.grid(3)
    cap, mask = I.cond()
    z3 = torch.cat([z, z[:1]])
    args = dict(cfg_scale=4.0, **ES.STEP_KW)
    from lumina_t2x_amd.transport import edit, integrators, path
    steps, last = integrators.sde_table(path.ICPlan(), "sigma", 1.0, torch.linspace(0, 0.96, 3), torch.tensor(0.48), "Heun", z, "Mean", 0.04, 0.96)
    steps[1, 2] = float("nan")  # the var of a stage record
    coef = integrators.views_guided_table(g3, torch.bfloat16, "fp32")
    refusals = [  # one argument refusal of each feature's list: an error code, nothing launched
        ("outside 0..3", lambda: model.forward(z, t, cap, mask, skip_layers=[9])),
        ("even batch", lambda: eng.sample_ode_cfg_schedule(z3, g3, [4.0, 4.0], "euler", **ES.STEP_KW)),
        ("finite and positive", lambda: eng.sample_ode_adaptive(z, g3, "dopri5", rtol=0.0, atol=0.0, use_cfg=True, **args)),
        ("cond - uncond difference", lambda: eng.forward_cfg_reuse(I.z[48][:, :, :16, :24].contiguous(), t, reuse=True, **args)),
        ("repeated", lambda: model.forward_with_cfg_slg(z, t, cap, mask, 4.0, slg_scale=2.0, slg_layers=[1, 1], **ES.STEP_KW)),
        (">= 0", lambda: model.sample_ode_teacache(z, g3, cap, mask, 4.0, threshold=-1.0, **ES.STEP_KW)),
        ("does not follow its probe", lambda: eng.forward_cached(z, t, "run", use_cfg=True, **args)),
        ("2 grid points", lambda: eng.sample_ode(z, [0.0], "euler", use_cfg=True, **args)),
        ("not finite", lambda: eng.sample_ode_cfg_rule(z, g3, [4.0, float("nan")], "euler", rescale=0.5, **ES.STEP_KW)),
        ("no views uploaded", lambda: eng.sample_views(I.z1[16], g3)),
        ("multistep", lambda: eng.sample_ode_masked(z, g3, z, z, z, "abm2", use_cfg=True, **args)),
        ("not finite and positive", lambda: eng.sample_sde(z, I.noise[16][:2], steps, last, "Heun", "Mean", use_cfg=True, **args)),
        # (the conditioning is prepared for 2 rows; one edited image evaluates 4)
        ("lt_prepare_prompt was called for batch 2, step has batch 4",
         lambda: eng.sample_flowedit(I.z1[16], g3, I.noise[16][:2, :1].contiguous(), edit.flowedit_scales(2, 1.5, 5.5), **ES.STEP_KW)),
        ("halves differ", lambda: eng.forward_cfg_packed([I.z1[16][0], I.z1[48][0, :, :16, :24].contiguous()], t, **args)),
        ("halves differ", lambda: eng.sample_ode_packed([I.z1[16][0], I.z1[48][0, :, :16, :24].contiguous()], g3, "euler", use_cfg=True, **args)),
        ("no views uploaded", lambda: eng.sample_views_guided(I.z1[16], I.z1[16].clone(), g3, coef, **args)),
    ]
    walk = ES.circuit(len(cat))
    assert len(refusals) <= len(walk)  # every refusal is made at least once
    lines = []
    for n, i in enumerate(walk):
        bad = _visit(golden_dir, "next", drv, cat[i])
        if bad is not None:
            lines.append(f"visit {n}: {cat[i].name} after the refusal '{refusals[(n - 1) % len(refusals)][0]}': {bad}")
        word, call = refusals[n % len(refusals)]
        with pytest.raises(_lib.LuminaLibError, match=word):
            call()
    assert not lines, "\n".join(lines)
