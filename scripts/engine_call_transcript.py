#!/usr/bin/env python3
"""What every C entry of the engine is given, call by call, on the tiny golden text model (tests/golden/nextdit_tiny.npz): a 16 x 16 latent,
batch 2, a 3-point grid, euler and midpoint (ab2 for the multistep entries), a packed list of a 16 x 16 and a 16 x 8 sample, a 16 x 24 canvas
of two windows and a table of two views.  ``eng.lib`` is replaced by a proxy that writes down, for each call through it, the entry's name,
every scalar, every field of an ``LtStepArgs`` passed by reference, the contents of every ctypes array and - for a pointer - whether it is
null, and then makes the call.  Every public ``forward*`` / ``sample_*`` / ``set_views`` / ``set_windows`` / ``set_softmax_rule`` method of
``DiTEngine`` is called, every ``forward_with_cfg_*`` front end and every routing branch of ``sample_ode_cfg_schedule`` of the model, and one
refused call per family of refusals, its message kept.  Prints one JSON document: the steps in order, each with its calls and a sha256 of its
result.  Two trees over one library that print the same document hand the library the same arguments (profiles/engine_binding/).

    python scripts/engine_call_transcript.py > transcript.json

Needs a GPU; not part of the test suite.  Uses public methods and ``eng.lib`` alone; reads nothing outside the repository."""
import ctypes as C
import hashlib
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lumina_t2x_amd  # noqa: E402,F401
from lumina_t2x_amd import models, views  # noqa: E402
from lumina_t2x_amd._lib import LtStepArgs, LuminaLibError  # noqa: E402
from lumina_t2x_amd.engine import EngineLimits  # noqa: E402
from lumina_t2x_amd.transport import edit, integrators, path  # noqa: E402
from oracle import synth  # noqa: E402


def describe(a):
    """one argument as JSON: a scalar as it is, an array by its contents, a pointer by whether it is null"""
    if a is None:
        return "null"
    if isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, bytes):
        return a.decode()
    if isinstance(a, C.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, C.Array):
        return ["ptr" if v else "null" for v in a] if a._type_ is C.c_void_p else list(a)
    if hasattr(a, "_obj"):  # byref(...)
        obj = a._obj
        if isinstance(obj, LtStepArgs):
            return {name: getattr(obj, name) for name, _ in obj._fields_}
        return {"ref": type(obj).__name__}
    if isinstance(a, C._Pointer):
        return "ptr" if a else "null"
    return {"other": type(a).__name__}


class Recorder:
    """stands in for ``eng.lib``: every entry looked up on it is the library's, behind a note of what it was given"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def entry(*args):
            self.calls.append({"entry": name, "args": [describe(a) for a in args]})
            return fn(*args)
        return entry


def digest(res):
    if res is None:
        return None
    if isinstance(res, torch.Tensor):
        return hashlib.sha256(res.detach().to("cpu", torch.float64).numpy().tobytes()).hexdigest()[:16]
    if isinstance(res, dict):
        return {k: digest(v) for k, v in res.items()}
    if isinstance(res, (list, tuple)):
        return [digest(v) for v in res]
    return res


def main():
    g = np.load(os.path.join(REPO, "tests", "golden", "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    model = models.NextDiT(**cfg.ctor_kwargs())
    model.load_state_dict(synth.synth_state_dict(cfg, seed=int(g["seed_w"])), strict=True)
    model = model.eval().to("cuda", torch.bfloat16)
    model.engine_limits = EngineLimits(max_batch=8, max_tokens=4096, max_text=256)  # room for every call: the engine is never replaced
    bf = dict(device="cuda", dtype=torch.bfloat16)
    cap = torch.from_numpy(g["cap"])[:2].to(**bf)
    mask = torch.from_numpy(g["mask"])[:2].cuda()
    cap4, mask4 = torch.cat([cap, cap.flip(0)]), torch.cat([mask, mask.flip(0)])
    gen = torch.Generator().manual_seed(5)
    rand = lambda *shape: torch.randn(*shape, generator=gen).to(**bf)  # noqa: E731
    z1 = rand(1, cfg.in_channels, 16, 16)
    z = z1.repeat(2, 1, 1, 1)
    noise = rand(2, 2, cfg.in_channels, 16, 16)
    keep = (rand(1, 1, 16, 16) > 0).to(torch.bfloat16).expand_as(z).contiguous()
    pair = [rand(cfg.in_channels, 16, 16), rand(cfg.in_channels, 16, 8)]
    canvas = rand(1, cfg.in_channels, 16, 24)
    t = torch.full((2,), 0.3, device="cuda")
    step = dict(proportional_attn=True, base_seqlen=16)
    g3 = torch.tensor([0.0, 0.4, 1.0])
    apg = dict(eta=0.0, momentum=-0.5, norm_threshold=15.0)
    windows = ([(0, 0), (0, 8)], (16, 16))

    eng = model.engine(z, cap.shape[1])
    rec = eng.lib = Recorder(eng.lib)
    steps = []

    def note(name, fn):
        first = len(rec.calls)
        row = {"step": name}
        try:
            row["sha"] = digest(fn())
        except (LuminaLibError, TypeError) as exc:
            row["refused"] = f"{type(exc).__name__}: {exc}"
        torch.cuda.synchronize()
        row["calls"] = rec.calls[first:]
        steps.append(row)

    # ---- the engine's own methods, the conditioning prepared for 2 rows ------------------------------------------------------------------
    note("prepare_prompt 2", lambda: eng.prepare_prompt(cap, mask))
    note("forward", lambda: eng.forward(z, t, use_cfg=False, **step))
    note("forward cfg", lambda: eng.forward(z, t, use_cfg=True, cfg_scale=4.0, **step))
    note("forward skip", lambda: eng.forward(z, t, use_cfg=False, skip_layers=(1,), **step))
    note("forward perturb", lambda: eng.forward(z, t, use_cfg=False, skip_layers=(1,), perturb_layers=(0,), **step))
    note("forward_packed", lambda: eng.forward_packed(pair, t, **step))
    for mode, tt in (("probe", t), ("run", t), ("probe", t * 0.5), ("reuse", t * 0.5)):
        note(f"forward_cached {mode}", lambda: eng.forward_cached(z, tt, mode, use_cfg=True, cfg_scale=4.0, **step))
    note("forward_cfg_slg", lambda: eng.forward_cfg_slg(z, t, cfg_scale=4.0, slg_scale=2.0, slg_layers=(1,), **step))
    note("forward_cfg_pag", lambda: eng.forward_cfg_pag(z, t, cfg_scale=4.0, pag_scale=2.0, pag_layers=(0,), skip_layers=(1,), **step))
    note("forward_cfg_rule", lambda: eng.forward_cfg_rule(z, t, cfg_scale=4.0, rescale=0.5, norm_limit=10.0, **step))
    note("forward_cfg_project apg", lambda: eng.forward_cfg_project(z, t, cfg_scale=4.0, apg=apg, **step))
    note("forward_cfg_project keep", lambda: eng.forward_cfg_project(z, t, cfg_scale=4.0, apg=apg, keep_momentum=True, **step))
    note("forward_cfg_project zero_star", lambda: eng.forward_cfg_project(z, t, cfg_scale=4.0, zero_star=True, **step))
    note("forward_cfg_reuse store", lambda: eng.forward_cfg_reuse(z, t, cfg_scale=4.0, **step))
    note("forward_cfg_reuse out=", lambda: eng.forward_cfg_reuse(z, t, cfg_scale=3.0, reuse=True, out=torch.empty_like(z), **step))
    for method, stages in (("euler", 1), ("midpoint", 2)):
        n = 2 * stages
        table = torch.tensor([4.0, 1.0, 2.5, 1.0][:n] if stages == 2 else [4.0, 1.0])
        third = [2.0, 0.0, 1.5, 1.0][:n] if stages == 2 else [2.0, 0.0]
        flags = torch.tensor([0, 1, 1, 0][:n] if stages == 2 else [0, 1], dtype=torch.int32)
        for traj in (True, False):
            note(f"sample_ode {method} traj={traj}", lambda: eng.sample_ode(z, g3, method, use_cfg=True, cfg_scale=4.0, return_trajectory=traj, **step))
        note(f"sample_ode_cached {method}", lambda: eng.sample_ode_cached(z, g3, method, use_cfg=True, threshold=1e9, cfg_scale=4.0, **step))
        note(f"sample_ode_masked {method}", lambda: eng.sample_ode_masked(z, g3, keep, z.flip(-1), noise[0], method, use_cfg=True, cfg_scale=4.0, **step))
        note(f"sample_ode_cfg_schedule {method}", lambda: eng.sample_ode_cfg_schedule(z, g3, table, method, **step))
        note(f"sample_ode_cfg_rule {method}", lambda: eng.sample_ode_cfg_rule(z, g3, table.tolist(), method, rescale=0.5, norm_limit=10.0, **step))
        note(f"sample_ode_cfg_project {method}", lambda: eng.sample_ode_cfg_project(z, g3, table, method, zero_star=True, zero_init=1, **step))
        note(f"sample_ode_cfg_reuse {method}", lambda: eng.sample_ode_cfg_reuse(z, g3, torch.full((n,), 3.0), flags, method, return_trajectory=False, **step))
        note(f"sample_ode_cfg_slg {method}", lambda: eng.sample_ode_cfg_slg(z, g3, table, third, (1,), method, **step))
        note(f"sample_ode_cfg_pag {method}", lambda: eng.sample_ode_cfg_pag(z, g3, table, third, (0,), method, skip_layers=(1,), **step))
    note("sample_ode_multistep", lambda: eng.sample_ode_multistep(z, g3, "ab2", use_cfg=True, cfg_scale=4.0, **step))
    note("sample_ode_multistep table", lambda: eng.sample_ode_multistep(z, g3, "ab2", use_cfg=True, table=[4.0, 1.0], rescale=0.5, **step))
    coef = torch.tensor([[0.0] * 4 + [1.0, 0.0, 0.0, 0.0], [0.0] * 4 + [1.5, -0.5, 0.0, 0.0]])
    note("sample_ode_multistep coef", lambda: eng.sample_ode_multistep(z, g3, None, use_cfg=True, cfg_scale=4.0, coef=coef, return_trajectory=False, **step))
    note("sample_ode_multistep_cfg_reuse", lambda: eng.sample_ode_multistep_cfg_reuse(z, g3, "ab2", [3.0, 3.0], [0, 1], **step))
    note("sample_ode_adaptive", lambda: eng.sample_ode_adaptive(z, g3, "dopri5", rtol=5e-2, atol=5e-2, use_cfg=True, cfg_scale=4.0, **step))
    sde_steps, sde_last = integrators.sde_table(path.ICPlan(), "sigma", 1.0, torch.linspace(0, 0.96, 3), torch.tensor(0.48), "Heun", z, "Mean", 0.04, 0.96)
    note("sample_sde", lambda: eng.sample_sde(z, noise, sde_steps, sde_last, "Heun", "Mean", use_cfg=True, cfg_scale=2.0, **step))
    note("sample_sde no last step", lambda: eng.sample_sde(z, noise, sde_steps[::2].contiguous(), None, "Euler", None, use_cfg=True, cfg_scale=2.0, **step))

    # ---- 4 rows: a packed list of 2 x 2 samples, the 4 branches of an edit, 2 views, 2 windows -------------------------------------------------
    quad = pair + [x.clone() for x in pair]
    note("prepare_prompt 4", lambda: eng.prepare_prompt(cap4, mask4))
    note("forward_cfg_packed", lambda: eng.forward_cfg_packed(quad, t.repeat(2), cfg_scale=4.0, **step))
    for traj in (True, False):
        note(f"sample_ode_packed traj={traj}", lambda: eng.sample_ode_packed(quad, g3, "euler", use_cfg=True, cfg_scale=4.0, return_trajectory=traj, **step))
    ones = [torch.ones_like(x) for x in quad]
    note("sample_ode_masked_packed", lambda: eng.sample_ode_masked_packed(quad, g3, ones, [x.flip(-1) for x in quad], [x * 0.5 for x in quad], "midpoint",
                                                                        use_cfg=True, cfg_scale=4.0, **step))
    note("sample_ode_multistep_packed", lambda: eng.sample_ode_multistep_packed(quad, g3, "ab2", use_cfg=True, cfg_scale=4.0, **step))
    note("sample_flowedit", lambda: eng.sample_flowedit(z1, g3, noise[:, :1].contiguous(), edit.flowedit_scales(2, 1.5, 5.5), **step))
    note("sample_views without views", lambda: eng.sample_views(z1, g3))
    note("set_views", lambda: eng.set_views([views.IdentityView(), views.Rotate180View()], 16, 16))
    note("sample_views", lambda: eng.sample_views(z1, g3, "midpoint", cfg_scale=4.0))
    note("set_softmax_rule anagram", lambda: eng.set_softmax_rule("anagram"))
    vcoef = integrators.views_guided_table(g3, torch.bfloat16, "fp32")
    note("sample_views_guided", lambda: eng.sample_views_guided(z1, z1.flip(-2).contiguous(), g3, vcoef, cfg_scale=4.0, scale_watershed=0.0, **step))
    note("set_softmax_rule t2i", lambda: eng.set_softmax_rule("t2i"))
    note("set_views None", lambda: eng.set_views(None, 0, 0))
    note("forward_tiled without windows", lambda: eng.forward_tiled(canvas, t.repeat(2)))
    note("set_windows", lambda: eng.set_windows(windows[0], windows[1], (16, 24), torch.full((16, 16), 0.5)))
    note("forward_tiled", lambda: eng.forward_tiled(canvas, t.repeat(2), cfg_scale=4.0, **step))
    note("sample_ode_tiled", lambda: eng.sample_ode_tiled(canvas, g3, "euler", cfg_scale=4.0, return_trajectory=False, **step))
    note("set_windows None", lambda: eng.set_windows(None, None, None))

    # ---- the model's front ends: every forward_with_cfg_* and every routing branch of sample_ode_cfg_schedule ----------------------------------
    note("model forward_with_cfg_rule off", lambda: model.forward_with_cfg_rule(z, t, cap, mask, 4.0, **step))
    note("model forward_with_cfg_rule", lambda: model.forward_with_cfg_rule(z, t, cap, mask, 4.0, rescale=0.5, norm_limit=10.0, **step))
    note("model forward_with_cfg_project off", lambda: model.forward_with_cfg_project(z, t, cap, mask, cfg_scale=4.0, **step))
    note("model forward_with_cfg_project", lambda: model.forward_with_cfg_project(z, t, cap, mask, 4.0, apg=apg, **step))
    note("model forward_with_cfg_reuse", lambda: model.forward_with_cfg_reuse(z, t, cap, mask, 4.0, **step))
    note("model forward_with_cfg_slg", lambda: model.forward_with_cfg_slg(z, t, cap, mask, 4.0, slg_scale=2.0, slg_layers=(1,), **step))
    note("model forward_with_cfg_pag", lambda: model.forward_with_cfg_pag(z, t, cap, mask, 4.0, pag_scale=2.0, pag_layers=(0,), **step))
    note("model forward_with_cfg_tiled", lambda: model.forward_with_cfg_tiled(canvas, 0.3, windows, cap, mask, 4.0, **step))
    note("model sample_ode_tiled", lambda: model.sample_ode_tiled(canvas, g3, windows, cap, mask, 4.0, method="euler", **step))
    note("model sample_ode_teacache", lambda: model.sample_ode_teacache(z, g3, cap, mask, 4.0, method="euler", threshold=1e9, **step))
    tab4, two = [4.0, 1.0, 2.5, 1.0], [4.0, 1.0]

    def route(tab, method="midpoint", **kw):
        return lambda: model.sample_ode_cfg_schedule(z, g3, tab, cap, mask, method=method, return_trajectory=True, **step, **kw)
    note("route schedule", route(tab4))
    note("route rule", route(tab4, rescale=0.5))
    note("route reuse", route([3.0] * 4, reuse=[0, 1, 1, 0]))
    note("route slg", route(tab4, slg=[2.0, 0.0, 1.5, 1.0], slg_layers=(1,)))
    note("route pag", route(tab4, pag=[2.0, 0.0, 1.5, 1.0], pag_layers=(0,), slg_layers=(1,)))
    note("route project", route(tab4, apg=apg))
    note("route multistep", route(two, "ab2", norm_limit=10.0))
    note("route multistep reuse", route([3.0, 3.0], "ab2", reuse=[0, 1]))

    # ---- refusals, one per family (the conditioning is the 2-row one again) ---------------------------------------------------------------
    note("refused: table length", lambda: eng.sample_ode_cfg_schedule(z, g3, [4.0, 1.0, 2.5], "midpoint", **step))
    note("refused: slg table length", lambda: eng.sample_ode_cfg_slg(z, g3, tab4, [2.0], (1,), "midpoint", **step))
    note("refused: pag table length", lambda: eng.sample_ode_cfg_pag(z, g3, two, [2.0], (0,), "midpoint", **step))
    note("refused: reuse table length", lambda: eng.sample_ode_cfg_reuse(z, g3, tab4, [0, 1], "midpoint", **step))
    note("refused: multistep table length", lambda: eng.sample_ode_multistep(z, g3, "ab2", use_cfg=True, table=tab4, **step))
    note("refused: unknown method", lambda: eng.sample_ode(z, g3, "heun3", use_cfg=True, **step))
    note("refused: unknown method, slg", lambda: eng.sample_ode_cfg_slg(z, g3, two, two, (1,), "ab2", **step))
    note("refused: unknown method, tiled", lambda: eng.sample_ode_tiled(canvas, g3, "ab2"))
    note("refused: list state", lambda: eng.sample_ode_cfg_project([z1[0]], g3, two, "euler", zero_star=True))
    note("refused: list state, model", lambda: model.forward_with_cfg_slg([z1[0]], t, cap, mask, 4.0, slg_scale=2.0, slg_layers=(1,)))
    note("refused: list state, route", lambda: model.sample_ode_cfg_schedule([z1[0]], g3, tab4, cap, mask, method="midpoint", slg=tab4,
                                                                            slg_layers=(1,), **step))
    note("refused: masked multistep", lambda: eng.sample_ode_masked(z, g3, keep, z, noise[0], "ab2", use_cfg=True, **step))
    note("refused: rule", lambda: eng.forward_cfg_rule(z, t, cfg_scale=4.0, rescale=2.0, **step))
    note("refused: no projected form", lambda: eng.forward_cfg_project(z, t, cfg_scale=4.0, **step))
    note("refused: out", lambda: eng.forward_cfg_reuse(z, t, cfg_scale=4.0, out=torch.empty_like(z1), **step))
    note("refused: guided skip", lambda: eng.forward(z, t, use_cfg=True, skip_layers=(1,), **step))
    note("refused: cpu state", lambda: eng.forward(z.cpu(), t, use_cfg=False))
    note("refused: needs cfg_scale", lambda: model.forward_with_cfg_pag(z, t, cap, mask, pag_scale=2.0, pag_layers=(0,), **step))
    note("refused: positional arguments", lambda: model.forward_with_cfg_reuse(z, t, cap, mask, 4.0, 1.0, **step))
    note("refused: rule with reuse", route(tab4, rescale=0.5, reuse=[0, 1, 1, 0]))

    assert model._engine is eng and eng.lib is rec, "the engine was replaced: its calls were not written down"
    print(json.dumps({"steps": steps}, indent=1), flush=True)


if __name__ == "__main__":
    main()
