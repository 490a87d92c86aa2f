"""Engine state tests: the catalogue of engine calls, the driver that applies their settings the way a long-lived user would, the Eulerian
circuit over a catalogue and the host model of the graph cache's FIFO rule (tests/test_engine_sequences_cpu.py, tests/test_gpu_engine_sequences.py).

An ``Entry`` is a name, the settings it needs (prompt, softmax rule, views, option overrides) and ``run(model, inputs) -> (tensors, ints)``.  Its
inputs are integer hashes of the element index: identical for every use, on every model.  Nothing here reads engine internals: what the driver
knows about the engine's persistent state (the stored cond - uncond difference of DESIGN 7k, the stored residual of DESIGN 7n) is a Python-side
restatement of the documented contract:

* every ``lt_prepare_prompt*`` / ``lt_prepare_labels`` call forgets both; the Python layer skips that call exactly when the conditioning tensors
  are the objects of the previous call and no ``set_option`` came since (``_SourceCache``);
* a refresh evaluation (``forward_with_cfg_reuse(reuse=False)``, a refresh stage of a reuse table) stores the difference with the signature
  ``(B', H, W, ch)``; a reuse is served when a difference of that signature is there, whatever calls came between, and refused by name
  otherwise;
* a run of the block stack under step caching (``forward_cached(..., "run")``, every run of ``sample_ode_teacache``) stores the residual with
  the signature ``(B, H, W, use_cfg)``; ``forward_cached(..., "reuse")`` behind its own probe is served on the same terms.

Not under test here: the step flags a guided call leaves on the Python MODULE for the plain ``forward`` that follows (the attention flags on the
layers, ``_rope`` / ``rope_scaling_factor`` / ``ntk_factor``), as the reference module does.  An entry that calls the plain ``forward`` sets them
itself first (``_plain_flags``), and guided entries pass every step flag explicitly, so an entry's result is a function of the entry; a
regression in how those flags are mirrored is for the feature tests to catch, not for the walk.  The samplers are entered through the
methods the transport front ends call (``model._engine_sample_*``)."""
import dataclasses
import math
from typing import Callable, Optional, Tuple

import torch

STEP_KW = dict(proportional_attn=True, base_seqlen=16)
SIZES = (16, 48)  # latent side: 2 x 64 = 128 rows run as plain launches, 2 x 576 = 1152 rows lie above the 1024-row graph threshold
LOUD_EXP = 12  # the loud entry's state is the hash times 2^12: finite under the torch model (tests/test_engine_sequences_cpu.py)
HUGE = 1e30


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def hashed(shape, seed, dtype=torch.float32):
    """values in [-1, 1) on a 2^-11 grid from an integer hash of the element index (no RNG)"""
    n = math.prod(shape)
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + (seed + 1) * 40503) % (1 << 32)
    h = h ^ (h >> 15)
    h = (h * 2246822519) % (1 << 32)
    h = h ^ (h >> 13)
    return ((h % 4096).to(torch.float32) / 2048.0 - 1.0).reshape(shape).to(dtype)


def grid(n, shift=4.0):
    """an n-point time grid with the samplers' time shift"""
    t = torch.linspace(0.0, 1.0, n)
    return t / (t + shift - shift * t)


class Inputs:
    """every tensor an entry of one family reads, built once per model device; ``cond`` is the family's golden conditioning"""

    def __init__(self, family, cond, device="cuda", cap_dim=128):
        self.family, self.device, self.text = family, device, len(cond) == 2
        dev = lambda t: t.to(device)  # noqa: E731
        self.z, self.zf, self.z1 = {}, {}, {}
        for s in SIZES:
            half = hashed((1, 4, s, s), 10 + s)
            self.z[s] = dev(half.repeat(2, 1, 1, 1).to(torch.bfloat16))
            self.zf[s] = dev(half.repeat(2, 1, 1, 1))
            self.z1[s] = dev(half.to(torch.bfloat16))
        self.t = dev(torch.tensor([0.3, 0.3]))
        self.prompts = {}
        if self.text:
            cap, mask = cond
            T = cap.shape[1]
            self.prompts["A"] = (cap, mask)
            self.prompts["A2"] = (dev(hashed(tuple(cap.shape), 3).to(cap.dtype)), mask.clone())
            mb = torch.ones(2, T + 8, dtype=mask.dtype)
            mb[1, 5:] = 0
            self.prompts["B"] = (dev(hashed((2, T + 8, cap_dim), 4).to(cap.dtype)), dev(mb))
            m4 = torch.ones(4, T, dtype=mask.dtype)
            m4[2:, 9:] = 0
            self.prompts["P4"] = (dev(hashed((4, T, cap_dim), 5).to(cap.dtype)), dev(m4))
        else:
            (y,) = cond
            self.prompts["A"] = (y,)
            self.prompts["A2"] = (dev(torch.tensor([7, int(y[-1])], dtype=y.dtype)),)
        self.noise = {s: dev(hashed((3, 2, 4, s, s), 20 + s).to(torch.bfloat16)) for s in SIZES}
        self.mask = {s: dev((hashed((1, 1, s, s), 30 + s) > 0).to(torch.bfloat16)) for s in SIZES}
        self.packed = {"small": [(16, 16), (24, 16)], "large": [(48, 48), (32, 40)]}

    def kw(self, prompt="A", guided=True, cfg_scale=4.0, **extra):
        """the keyword arguments of the family's forward_with_cfg (guided) or forward"""
        names = ("cap_feats", "cap_mask") if self.text else ("y",)
        kw = dict(zip(names, self.prompts[prompt]))
        if guided:
            kw["cfg_scale"] = cfg_scale
            if self.family in ("next", "flag"):
                kw.update(STEP_KW)
            if self.family != "next":
                kw.update(rope_scaling_factor=1.0, ntk_factor=1.0)
        kw.update(extra)
        return kw

    def cond(self, prompt="A"):
        return self.prompts[prompt]

    def packed_list(self, which):
        half = [hashed((4, h, w), 40 + h + w).to(torch.bfloat16).to(self.device) for h, w in self.packed[which]]
        return half + [x.clone() for x in half]

    def ensure_engine(self, model):
        z = self.z[16]
        return model.engine(z, self.prompts["A"][0].shape[1]) if self.text else model.engine(z)


# ---- entries -------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Entry:
    name: str
    methods: Tuple[str, ...]  # model / engine methods the entry goes through (tests/test_gpu_engine_sequences.py counts the calls: all are made)
    size: int  # latent side; 0: a packed size list
    run: Callable
    prompt: str = "A"
    rule: str = "t2i"
    views: Optional[int] = None  # the latent side the two view tables are built for
    options: Tuple[Tuple[str, int], ...] = ()
    # graph keys the entry certainly uses, as labels (a lower bound: evaluations above 1024 rows that differ in a word of lt_step_args - cfg_scale,
    # io dtype, batch, scale_factor - or of extra[]: the prompt's shape, the softmax rule, the closing kernel, the segment, the skip set, the size list)
    keys: Tuple = ()
    stores: Optional[Tuple] = None  # ("delta" | "residual", signature) it leaves behind
    needs: Optional[Tuple] = None  # ("delta" | "residual", signature, words of the refusal without it)


def _plain_flags(model, I):
    """what a forward_with_cfg with these step flags leaves on the module for the plain forward that follows"""
    if I.family in ("next", "flag"):
        model._mirror_attention_flags(dict(STEP_KW))
    if I.family == "flag":
        model.rope_scaling_factor, model.ntk_factor = 1.0, 1.0
    elif I.family != "next":
        model._rope = (1.0, 1.0)


def _counters(model, cache=False):
    eng = model._engine
    out = (eng.last_nfe(), eng.last_eval_rows(), eng.get_option("layout_flips"))
    return out + (eng.last_cache_hits(),) if cache else out


def _eng_args(model, I, z, guided=True, prompt="A"):
    kw = I.kw(prompt, guided)
    if guided:
        model._mirror_attention_flags(kw)
    else:
        _plain_flags(model, I)
    return model._engine_sampler_args(z, guided, kw)


def _views(s):
    from lumina_t2x_amd import views
    return [views.IdentityView(), views.Rotate180View()]


def _size_entries(s, family):
    """the entries every family can serve at latent side s"""
    big = s == 48
    K = lambda *k: ((family, s) + k,) if big else ()  # noqa: E731
    cfg_key = K("cfg", 4.0, "bf16")
    e = {}

    def add(name, methods, run, **kw):
        e[name] = Entry(f"{name}@{s}", tuple(methods), s, run, **kw)

    def fwd(m, I):
        _plain_flags(m, I)
        return (m.forward(I.z[s], I.t, *I.cond()),), ()
    add("forward", ["forward"], fwd, keys=K("plain"))
    add("cfg_bf16", ["forward_with_cfg"], lambda m, I: ((m.forward_with_cfg(I.z[s], I.t, **I.kw()),), ()), keys=cfg_key)
    add("cfg_fp32", ["forward_with_cfg"], lambda m, I: ((m.forward_with_cfg(I.zf[s], I.t, **I.kw()),), ()), keys=K("cfg", 4.0, "fp32"))

    def skip(m, I):
        _plain_flags(m, I)
        return (m.forward(I.z[s], I.t, *I.cond(), skip_layers=(1, 2)),), ()
    add("forward_skip", ["forward"], skip, keys=K("plain", "skip", (1, 2)))

    def ode(method):
        return lambda m, I: ((m._engine_sample_ode(I.z[s], grid(3), method, True, True, I.kw()),), _counters(m))
    for method in ("euler", "midpoint", "rk4"):
        add(f"ode_{method}", ["_engine_sample_ode", "sample_ode"], ode(method), keys=cfg_key)

    def sched(m, I):
        out = m.sample_ode_cfg_schedule(I.z[s], grid(3), [4.0, 1.0, 3.0, 2.5], *I.cond(), method="midpoint", return_trajectory=True, **_step_kw(I))
        return (out,), _counters(m)
    add("cfg_schedule", ["sample_ode_cfg_schedule"], sched, keys=K("dev", "guided"))

    def reuse_traj(m, I):
        out = m.sample_ode_cfg_schedule(I.z[s], grid(3), [4.0, 3.0, 1.0, 2.5], *I.cond(), method="midpoint", return_trajectory=True,
                                        reuse=[0, 1, 0, 1], **_step_kw(I))
        return (out,), _counters(m)
    add("cfg_reuse_traj", ["sample_ode_cfg_schedule", "sample_ode_cfg_reuse"], reuse_traj, keys=K("dev", "store"), stores=("delta", (1, s, s, 3)))
    add("cfg_reuse_store", ["forward_with_cfg_reuse", "forward_cfg_reuse"],
        lambda m, I: ((m.forward_with_cfg_reuse(I.z[s], I.t, *I.cond(), 4.0, reuse=False, **_step_kw(I)),), ()), keys=K("dev", "store"),
        stores=("delta", (1, s, s, 3)))
    add("cfg_reuse_use", ["forward_with_cfg_reuse", "forward_cfg_reuse"],
        lambda m, I: ((m.forward_with_cfg_reuse(I.z[s], I.t, *I.cond(), 3.0, reuse=True, **_step_kw(I)),), ()),
        needs=("delta", (1, s, s, 3), ("lt_forward_cfg_reuse", "cond - uncond difference")))

    def slg_traj(m, I):
        out = m.sample_ode_cfg_schedule(I.z[s], grid(3), [4.0, 1.0, 1.0, 3.0], *I.cond(), method="midpoint", return_trajectory=True,
                                        slg=[2.8, 0.0, 1.5, 0.0], slg_layers=[2, 1], **_step_kw(I))
        return (out,), _counters(m)
    add("slg_traj", ["sample_ode_cfg_schedule", "sample_ode_cfg_slg"], slg_traj, keys=K("dev", "slg_guided"))

    def tea(thr):
        def run(m, I):
            k = I.kw()
            cfg_scale = k.pop("cfg_scale")
            cond = [k.pop(n) for n in m._cond_names]
            out = m.sample_ode_teacache(I.z[s], grid(4), *cond, cfg_scale, method="euler", threshold=thr, return_trajectory=True, **k)
            return (out,), _counters(m, cache=True)
        return run
    res = ("residual", (2, s, s, 1))
    seg = K("cfg", "head") + K("cfg", "blocks")
    add("teacache_0", ["sample_ode_teacache", "sample_ode_cached"], tea(0.0), keys=seg, stores=res)
    add("teacache_huge", ["sample_ode_teacache", "sample_ode_cached"], tea(HUGE), keys=seg + K("cfg", "apply"), stores=res)

    def cached(m, I):
        eng, a = _eng_args(m, I, I.z[s])
        eng.forward_cached(I.z[s], I.t, "probe", use_cfg=True, **a)
        ran = eng.forward_cached(I.z[s], I.t, "run", use_cfg=True, **a)
        sums = eng.forward_cached(I.z[s], I.t * 0.5, "probe", use_cfg=True, **a)  # against the first probe of this entry
        again = eng.forward_cached(I.z[s], I.t * 0.5, "reuse", use_cfg=True, **a)
        return (ran, again, torch.tensor(sums, dtype=torch.float64)), ()
    add("cached_probe_run_reuse", ["forward_cached"], cached, keys=seg + K("cfg", "apply"), stores=res)

    def cached_reuse(m, I):
        eng, a = _eng_args(m, I, I.z[s])
        eng.forward_cached(I.z[s], I.t * 0.25, "probe", use_cfg=True, **a)
        return (eng.forward_cached(I.z[s], I.t * 0.25, "reuse", use_cfg=True, **a),), ()
    add("cached_reuse", ["forward_cached"], cached_reuse, needs=res + (("lt_forward_cached", "without a stored residual"),))
    return e


def _step_kw(I):
    k = I.kw()
    for n in ("cap_feats", "cap_mask", "y", "cfg_scale"):
        k.pop(n, None)
    return k


def _next_entries(s):
    big = s == 48
    K = lambda *k: (("next", s) + k,) if big else ()  # noqa: E731
    cfg_key = K("cfg", 4.0, "bf16")
    e = _size_entries(s, "next")

    def add(name, methods, run, **kw):
        e[name] = Entry(f"{name}@{s}", tuple(methods), s, run, **kw)

    def dopri5(m, I):
        out, st = m._engine_sample_ode_adaptive(I.z[s], grid(3), "dopri5", True, True, I.kw(), rtol=5e-2, atol=5e-2)
        return (out,), _counters(m) + (st["nfe"], st["accepted"], st["rejected"])
    add("dopri5", ["_engine_sample_ode_adaptive", "sample_ode_adaptive"], dopri5, keys=cfg_key)
    add("abm3", ["_engine_sample_ode_multistep", "sample_ode_multistep"],
        lambda m, I: ((m._engine_sample_ode_multistep(I.zf[s], grid(4), "abm3", True, True, I.kw(cfg_scale=3.0)),), _counters(m)),
        keys=K("cfg", 3.0, "fp32"))

    def rule(m, I):
        out = m.sample_ode_cfg_schedule(I.z[s], grid(3), [4.0, 3.0, 1.0, 2.5], *I.cond(), method="midpoint", return_trajectory=True, rescale=0.5,
                                        norm_limit=2.0, **_step_kw(I))
        return (out,), _counters(m)
    add("cfg_rule", ["sample_ode_cfg_schedule", "sample_ode_cfg_rule"], rule, keys=K("dev", "rule"))
    add("slg_forward", ["forward_with_cfg_slg", "forward_cfg_slg"],
        lambda m, I: ((m.forward_with_cfg_slg(I.z[s], I.t, *I.cond(), 4.0, slg_scale=2.8, slg_layers=[1, 2], **STEP_KW),), ()),
        keys=K("dev", "slg_guided"))

    def sde(m, I):
        from lumina_t2x_amd.transport import integrators, path
        z = I.z[s]
        steps, last = integrators.sde_table(path.ICPlan(), "sigma", 1.0, torch.linspace(0, 0.96, 3), torch.tensor(0.48), "Heun", z, "Mean", 0.04, 0.96)
        _, traj, final = m._engine_sample_sde(z, I.noise[s][:2], steps, last, "Heun", "Mean", True, I.kw(cfg_scale=2.0))
        return (traj, final), _counters(m)
    add("sde", ["_engine_sample_sde", "sample_sde"], sde, keys=K("cfg", 2.0, "bf16"))

    def masked(m, I):
        z = I.z[s]
        out = m.sample_ode_masked(z, grid(3), I.mask[s], I.z1[s].flip(-1), I.noise[s][2, :1], *I.cond(), 5.0, method="midpoint", return_trajectory=True,
                                  **STEP_KW)
        return (out,), _counters(m)
    add("masked", ["sample_ode_masked"], masked, keys=K("cfg", 5.0, "bf16"))

    def flowedit(m, I):
        out = m.sample_flowedit(I.z1[s], grid(3), I.noise[s][:2, :1].contiguous(), *I.cond("P4"), src_cfg=1.5, tgt_cfg=5.5, return_trajectory=True,
                                **STEP_KW)
        return (out,), _counters(m)
    add("flowedit", ["sample_flowedit"], flowedit, prompt="P4", keys=K("plain", "rows4"))

    def views_init(m, I):
        eng = m.engine(I.z1[s].expand(4, -1, -1, -1), I.cond("P4")[0].shape[1])
        eng.prepare_prompt(*I.cond("P4"))
        return (eng.sample_views(I.z1[s], grid(3), "midpoint", cfg_scale=4.0),), _counters(m)
    add("views", ["sample_views", "set_views", "set_softmax_rule"], views_init, prompt="P4", rule="anagram", views=s, keys=K("cfg", "views"))

    def views_guided(m, I):
        from lumina_t2x_amd.transport.integrators import views_guided_table
        eng = m.engine(I.z1[s].expand(4, -1, -1, -1), I.cond("P4")[0].shape[1])
        eng.prepare_prompt(*I.cond("P4"))
        m._mirror_attention_flags(dict(STEP_KW))
        coef = views_guided_table(grid(3), torch.bfloat16, "fp32")
        out = eng.sample_views_guided(I.z1[s], I.z1[s].flip(-2).contiguous(), grid(3), coef, cfg_scale=4.0, scale_watershed=0.0, **STEP_KW)
        return (out,), _counters(m)
    add("views_guided", ["sample_views_guided", "set_views", "set_softmax_rule"], views_guided, prompt="P4", rule="anagram", views=s,
        keys=K("cfg", "views", "prop"))
    return e


def _next_catalogue():
    out = []
    for s in SIZES:
        out += list(_next_entries(s).values())

    def add(name, methods, size, run, **kw):
        out.append(Entry(name, tuple(methods), size, run, **kw))

    t4 = lambda I: I.t.repeat(2)  # noqa: E731
    for which, rows in (("small", 4 * 96), ("large", 4 * 576)):
        assert (rows <= 1024) == (which == "small")
        key = (("next", "packed", which),) if which == "large" else ()
        add(f"packed_cfg_{which}", ["forward_with_cfg_packed", "forward_cfg_packed"], 0,
            (lambda w: lambda m, I: (tuple(m.forward_with_cfg_packed(I.packed_list(w), t4(I), *I.cond("P4"), 4.0, **STEP_KW)), ()))(which),
            prompt="P4", keys=key)
        add(f"packed_ode_{which}", ["sample_ode_packed"], 0,
            (lambda w: lambda m, I: (tuple(m.sample_ode_packed(I.packed_list(w), grid(3), *I.cond("P4"), 4.0, method="euler", return_trajectory=True,
                                                                **STEP_KW)), _counters(m)))(which), prompt="P4", keys=key)
    add("prompt_B@48", ["forward_with_cfg"], 48, lambda m, I: ((m.forward_with_cfg(I.z[48], I.t, **I.kw("B")),), ()), prompt="B",
        keys=(("next", 48, "cfg", "prompt_B"),))
    add("prompt_A2@48", ["forward_with_cfg"], 48, lambda m, I: ((m.forward_with_cfg(I.z[48], I.t, **I.kw("A2")),), ()), prompt="A2")
    add("rope_scale_2@48", ["forward_with_cfg"], 48, lambda m, I: ((m.forward_with_cfg(I.z[48], I.t, **I.kw(scale_factor=2.0, scale_watershed=0.5)),), ()),
        keys=(("next", 48, "cfg", "scale_factor_2"),))
    add("loud@48", ["forward_with_cfg"], 48, lambda m, I: ((m.forward_with_cfg(I.z[48] * float(2 ** LOUD_EXP), I.t, **I.kw()),), ()))
    return out


def _family_catalogue(family):
    """the shorter catalogues: only what the family's front end serves, both sizes, guided and unguided evaluations"""
    e16, e48 = _size_entries(16, family), _size_entries(48, family)
    out = [e16["forward"], e48["forward"], e16["cfg_bf16"], e48["cfg_bf16"], e48["ode_midpoint"], e16["teacache_huge"]]
    if family == "imagenet":  # labels
        out.append(Entry("labels_2@48", ("forward_with_cfg", "prepare_labels"), 48, lambda m, I: ((m.forward_with_cfg(I.z[48], I.t, **I.kw("A2")),), ()),
                         prompt="A2"))
        out.append(e16["cfg_schedule"])
    elif family == "flag":  # eol tokens (every entry), ntk_factor
        out.append(Entry("ntk_2@48", ("forward_with_cfg",), 48, lambda m, I: ((m.forward_with_cfg(I.z[48], I.t, **I.kw(ntk_factor=2.0)),), ()),
                         keys=(("flag", 48, "cfg", "ntk2"),)))
        out.append(e16["slg_traj"])
    else:  # moe: the hoisted time plans (moe_tp_live) on and off
        out.append(Entry("no_hoist@48", ("forward_with_cfg",), 48, lambda m, I: ((m.forward_with_cfg(I.z[48], I.t, **I.kw()),), ()),
                         options=(("moe_time_plan_hoist", 0),), keys=(("moe", 48, "cfg", "no_hoist"),)))
        out.append(dataclasses.replace(e16["forward"], name="no_hoist_forward@16", options=(("moe_time_plan_hoist", 0),)))
    return out


CATALOGUES = {"next": _next_catalogue(), "imagenet": _family_catalogue("imagenet"), "flag": _family_catalogue("flag"), "moe": _family_catalogue("moe")}


def distinct_keys(entries):
    """a lower bound of the graph keys a catalogue uses"""
    return len({k for e in entries for k in e.keys})


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
class Refused:
    """the engine refused the call; ``message`` is its error text, which names the cause"""

    def __init__(self, message):
        self.message = message


class Driver:
    """applies an entry's settings to a model's engine only where they differ from what it was last given, runs the entry, and keeps the
    Python-side account of the documented contract (module docstring).  ``base_options``: overrides under every entry's own."""

    def __init__(self, model, inputs, base_options=()):
        self.model, self.I = model, inputs
        self.eng = inputs.ensure_engine(model)
        self.prompt = self.views = None
        self.rule = "t2i"
        self.options = {}
        self.base = dict(base_options)
        self.dirty = False  # an option changed since the last call: the next call prepares its conditioning again
        self.kept = {"delta": None, "residual": None}  # kind -> (signature, the entry that stored it)
        self._apply_options({})

    def set_base_options(self, base_options):
        self.base = dict(base_options)

    def _apply_options(self, own):
        want = dict(self.base, **own)
        for name in set(self.options) | set(want):
            if self.options.get(name) != want.get(name):
                self.eng.set_option(name, want.get(name))
                self.dirty = True
        self.options = want

    def apply(self, entry):
        assert self.model._engine is self.eng, "the engine was replaced: the limits given up front do not hold this entry"
        self._apply_options(dict(entry.options))
        if entry.rule != self.rule:
            self.eng.set_softmax_rule(entry.rule)
            self.rule = entry.rule
        if entry.views != self.views:
            self.eng.set_views(_views(entry.views) if entry.views else None, entry.views or 0, entry.views or 0)
            self.views = entry.views
        if entry.prompt != self.prompt or self.dirty:  # the call prepares its conditioning: difference and residual are forgotten
            self.kept = {"delta": None, "residual": None}
        self.prompt, self.dirty = entry.prompt, False

    def expectation(self, entry):
        """None: the entry does not depend on what came before; else ("served", storing entry) or ("refused", words)"""
        if entry.needs is None:
            return None
        kind, sig, words = entry.needs
        have = self.kept[kind]
        if have is not None and have[0] == sig:
            return ("served", have[1])
        return ("refused", words)

    def run(self, entry):
        """(tensors, ints), or Refused"""
        from lumina_t2x_amd._lib import LuminaLibError
        self.apply(entry)
        try:
            out = entry.run(self.model, self.I)
        except LuminaLibError as exc:
            return Refused(str(exc))
        if entry.stores is not None:
            self.kept[entry.stores[0]] = (entry.stores[1], entry)
        return out


# ---- circuit and FIFO ------------------------------------------------------------------------------------------------------------------------
def circuit(n):
    """an Eulerian circuit of the complete directed graph on n nodes with self-loops: n^2 + 1 visits, every ordered pair adjacent exactly once
    (Hierholzer on the fixed adjacency order 0 .. n-1)"""
    nxt = [0] * n
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            nxt[v] += 1
            stack.append(nxt[v] - 1)
        else:
            out.append(stack.pop())
    return out[::-1]


def fifo_replays(keys, cap=16):
    """the growth of graph_replays over a sequence of graph keys under the rule of forward_graphed_body: a key's first use runs eagerly, its
    second captures and replays, later ones replay; a new key drops the oldest of ``cap`` held ones, and a dropped key starts over"""
    held, replays = [], 0  # [key, uses], oldest first
    for k in keys:
        slot = next((h for h in held if h[0] == k), None)
        if slot is None:
            if len(held) >= cap:
                held.pop(0)
            slot = [k, 0]
            held.append(slot)
        replays += slot[1] > 0
        slot[1] += 1
    return replays
