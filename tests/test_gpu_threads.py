"""-m gpu: two engines on two threads and two streams equal their serial runs, word for word.

What include/lumina_dit.h and csrc/options.h promise and nothing else checked: engines with different settings can be driven from
different threads; lt_engine_set_option / lt_set_option are safe against a call running on an engine, which finishes on the snapshot of
all options it took at entry; an engine can be called from any thread.  Two calls at once on the SAME engine are promised nowhere and
are not made here; neither are concurrent lt_op_* calls (include/lumina_dit_debug.h: they share scratch space).

Every test is one process with at most three Python threads (the main one included).  A worker runs inside a torch.cuda.Stream() of
its own, workers start together on a barrier, what they raise is re-raised on the main thread, and a join that expires fails the test.
Serial baselines are recorded first, on the same engines with the same inputs; every comparison is torch.equal.  Nothing is asserted
about time.  Models: the two-layer tiny goldens of test_gpu_model.py / test_gpu_variants.py.
"""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models, views
from lumina_t2x_amd.transport import Sampler, create_transport
from oracle import synth

from gpu_util import lib, ok, set_option

pytestmark = pytest.mark.gpu

CALLS = 16           # per worker: with models this small the two loops overlap from the first call to the last
JOIN_TIMEOUT = 300.0  # generous: a join that expires is a hang, and fails the test
NEXT_KW = dict(base_seqlen=16, proportional_attn=True)


def _golden(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    return g, synth.NextDiTConfig(**json.loads(str(g["config"])))


def _build(ctor, cfg, seed):
    m = ctor(**cfg.ctor_kwargs())
    m.load_state_dict(synth.synth_state_dict(cfg, seed=seed), strict=True)
    return m.eval().to("cuda", torch.bfloat16)


class _Case:
    """one model with its golden inputs: ``fwd()`` = forward_with_cfg at scale 4, ``traj()`` = the 4-step Euler trajectory through the sampler
    API - the two calls a worker alternates"""

    def __init__(self, golden_dir, family):
        name, ctor = {"next": ("nextdit_tiny", models.NextDiT), "imagenet": ("imagenet_tiny", models.imagenet.DiT_Llama),
                      "moe": ("moe_tiny", models.moe.DiT_Llama)}[family]
        g, cfg = _golden(golden_dir, name)
        assert cfg.n_layers >= 2  # (a mixture of two option values shows only if more than one layer reads the option)
        self.family, self.model = family, _build(ctor, cfg, int(g["seed_w"]))
        self.z = torch.from_numpy(g["z"]).to("cuda", torch.bfloat16)
        self.t = torch.from_numpy(g["t"]).cuda()
        if family == "next":
            self.cond = dict(cap_feats=torch.from_numpy(g["cap"]).to("cuda", torch.bfloat16), cap_mask=torch.from_numpy(g["mask"]).cuda())
            self.kw = dict(NEXT_KW)
        else:
            self.cond, self.kw = dict(y=torch.from_numpy(g["y"]).cuda()), {}
        self.ode = Sampler(create_transport()).sample_ode(sampling_method="euler", num_steps=5)
        self.fwd()  # the engine exists from here on
        self.engine = self.model._engine

    def fwd(self):
        return self.model.forward_with_cfg(self.z, self.t, *self.cond.values(), 4.0, **self.kw)

    def traj(self):
        return self.ode(self.z, self.model.forward_with_cfg, cfg_scale=4.0, **self.cond, **self.kw)

    def call(self, i):
        return self.traj() if i % 2 else self.fwd()

    def baselines(self):
        """[forward_with_cfg, trajectory], each run three times: under "graph" 1 that is the eager run, the capture and a replay"""
        base = []
        for fn in (self.fwd, self.traj):
            outs = [fn() for _ in range(3)]
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "the serial runs disagree among themselves"
            base.append(outs[0].clone())
        assert base[1].shape[0] == 5 and not torch.equal(base[1][0], base[1][-1])
        return base


def _run_workers(workers, main=None):
    """``workers``: functions, one thread and one stream each; ``main`` (optional) runs on the calling thread once all have started"""
    torch.cuda.synchronize()  # the baselines ran on this thread's stream
    barrier = threading.Barrier(len(workers) + 1)
    errors = []

    def wrap(fn):
        def go():
            try:
                stream = torch.cuda.Stream()
                with torch.cuda.stream(stream):
                    barrier.wait(JOIN_TIMEOUT)
                    fn()
                    stream.synchronize()
            except BaseException as exc:  # noqa: BLE001 - re-raised on the main thread
                errors.append(exc)
                barrier.abort()
        return go

    threads = [threading.Thread(target=wrap(fn), daemon=True) for fn in workers]
    for th in threads:
        th.start()
    try:
        barrier.wait(JOIN_TIMEOUT)
        if main is not None:
            main()
    except threading.BrokenBarrierError:
        pass  # a worker failed before the start: its exception is in `errors`
    finally:
        for th in threads:
            th.join(JOIN_TIMEOUT)
    assert not any(th.is_alive() for th in threads), "a worker did not finish: a hang"
    if errors:
        raise errors[0]
    torch.cuda.synchronize()


def _alternating_worker(case, base, replays=None):
    """CALLS calls, forward_with_cfg and the trajectory in turn, every output kept and compared with its baseline after the loop (a
    comparison inside it would drain the stream between calls)"""
    def work():
        outs = []
        for i in range(CALLS):
            outs.append(case.call(i))
            if replays is not None:
                replays.append(case.engine.graph_replays())
        for i, o in enumerate(outs):
            assert torch.equal(o, base[i % 2]), f"{case.family} engine, concurrent call {i} ({'trajectory' if i % 2 else 'forward_with_cfg'}) left its serial baseline"
    return work


def _new_generation(engine):
    """re-state the engine's "graph" override: a new option generation, so the next calls run eagerly, capture and replay again"""
    engine.set_option("graph", engine.get_option("graph"))


@pytest.mark.parametrize("family,graph", [("moe", None), ("moe", 1), ("imagenet", 1)], ids=["moe-defaults", "moe-graph1", "imagenet-graph1"])
def test_independent_engines_on_two_threads(golden_dir, family, graph):
    """A: Next-DiT tiny, eager launches and the baseline attention kernel, for itself only.  B: another family - with the defaults, and
    with "graph" 1: the default, 2, replays above 1024 rows only and these models have 128, so the case that makes B capture and replay
    while A launches sets it for B alone.  B's captures happen INSIDE the concurrent phase (a new option generation just before it)."""
    a, b = _Case(golden_dir, "next"), _Case(golden_dir, family)
    a.engine.set_option("graph", 0)
    a.engine.set_option("attention_variant", 1)
    if graph is not None:
        b.engine.set_option("graph", graph)
    base_a, base_b = a.baselines(), b.baselines()
    if graph is not None:
        _new_generation(b.engine)
    ra, rb = a.engine.graph_replays(), b.engine.graph_replays()
    replays_b = []
    _run_workers([_alternating_worker(a, base_a), _alternating_worker(b, base_b, replays_b)])
    assert a.engine.graph_replays() == ra  # A's own override held while B replayed next to it
    assert replays_b == sorted(replays_b)
    if graph == 1:
        assert replays_b[-1] > rb, "B never replayed: the concurrent phase did not exercise capture and replay"
    else:
        assert replays_b[-1] == rb
    assert a.engine.get_option("attention_variant") == 1 and b.engine.get_option("attention_variant") == 4
    for case, base in ((a, base_a), (b, base_b)):  # and serially once more
        assert torch.equal(case.fwd(), base[0]) and torch.equal(case.traj(), base[1])


def test_same_family_two_overrides_with_allocation_inside_entry_points(golden_dir):
    """two Next-DiT tiny engines of one config.  A replays a graph it captures inside the concurrent phase and runs the ping-pong attention
    kernel; B launches eagerly and ALLOCATES inside entry points meanwhile: lt_set_views frees and allocates its five tables at every call,
    and B's first packed call ever allocates the engine's packed table.  A capture broken by the other thread's allocation would come
    back as an error here (the engine captures in thread-local mode).  The packed call's baseline is the tensor forward_with_cfg: at equal
    sizes the two are bit-identical (test_gpu_packed_cfg.py), so the call itself can stay unmade until the workers run."""
    a, b = _Case(golden_dir, "next"), _Case(golden_dir, "next")
    a.engine.set_option("graph", 1)
    a.engine.set_option("attention_variant", 3)
    b.engine.set_option("graph", 0)
    base_a, base_b = a.baselines(), b.baselines()
    tables = views.stack_tables([views.FlipView()], 16, 16, 4)
    grid = torch.tensor([0.0, 0.5, 1.0])
    z1 = b.z[:1].contiguous()

    def views_call():
        b.engine.set_views(tables, 16, 16)
        b.engine.prepare_prompt(*b.cond.values())
        return b.engine.sample_views(z1, grid, "euler", cfg_scale=4.0, **NEXT_KW)

    base_views = views_call()
    assert torch.equal(views_call(), base_views) and not torch.equal(base_views[-1], base_views[0])
    _new_generation(a.engine)
    ra = a.engine.graph_replays()

    def worker_b():
        outs = []
        for i in range(CALLS):
            if i % 4 == 1:
                outs.append(torch.stack(b.model.forward_with_cfg_packed(list(b.z), b.t, *b.cond.values(), 4.0, **b.kw)))
            elif i % 2:
                outs.append(views_call())
            else:
                outs.append(b.fwd())
        for i, o in enumerate(outs):
            want = base_b[0] if i % 2 == 0 or i % 4 == 1 else base_views
            assert torch.equal(o, want), f"engine B, concurrent call {i} left its serial baseline"

    replays_a = []
    _run_workers([_alternating_worker(a, base_a, replays_a), worker_b])
    assert replays_a == sorted(replays_a) and replays_a[-1] > ra, "A never replayed: no capture ran next to B's allocations"
    assert b.engine.graph_replays() == 0
    assert torch.equal(a.fwd(), base_a[0]) and torch.equal(a.traj(), base_a[1])
    assert torch.equal(b.fwd(), base_b[0]) and torch.equal(b.traj(), base_b[1]) and torch.equal(views_call(), base_views)
    assert torch.equal(torch.stack(b.model.forward_with_cfg_packed(list(b.z), b.t, *b.cond.values(), 4.0, **b.kw)), base_b[0])


@pytest.mark.parametrize("level", ["engine", "process"])
def test_option_flipped_under_a_running_call(golden_dir, level):
    """the ImageNet tiny (two layers) loops forward_with_cfg on a worker; the main thread flips "attn_small_fused" as fast as it can - the
    engine's override (lt_engine_set_option), or the process default (lt_set_option) of an engine without one.  The two settings give
    different words, and every layer reads the option: an output is the "0" baseline or the "1" baseline, whole.  Anything else means a
    layer read the option live instead of from the call's snapshot.  How many outputs match which is a matter of timing: printed only."""
    c = _Case(golden_dir, "imagenet")
    L, h = lib(), c.engine.handle
    base = {}
    try:
        for v in (0, 1):
            c.engine.set_option("attn_small_fused", v)
            outs = [c.fwd() for _ in range(2)]
            assert torch.equal(outs[0], outs[1])
            base[v] = outs[0].clone()
        assert not torch.equal(base[0], base[1]), "attn_small_fused changes nothing at this shape: the test could not see a mixture"
        if level == "process":
            c.engine.set_option("attn_small_fused", None)
        calls, outs, done, flips = 3 * CALLS, [], threading.Event(), [0]

        def worker():
            try:
                for _ in range(calls):
                    outs.append(c.fwd())
            finally:
                done.set()

        def flipper():
            name = b"attn_small_fused"
            while not done.is_set():
                v = flips[0] & 1
                ok(L.lt_engine_set_option(h, name, v) if level == "engine" else L.lt_set_option(name, v), "flip")
                flips[0] += 1

        _run_workers([worker], flipper)
    finally:
        set_option("attn_small_fused", 1)
        c.engine.set_option("attn_small_fused", None)
    assert len(outs) == calls
    match = [sum(torch.equal(o, base[v]) for o in outs) for v in (0, 1)]
    print(f"attn_small_fused flipped {flips[0]} times at the {level} level under {calls} calls: {match[0]} outputs equal the '0' baseline, "
          f"{match[1]} the '1' baseline")
    for i, o in enumerate(outs):
        assert torch.equal(o, base[0]) or torch.equal(o, base[1]), f"call {i} is neither baseline: a layer read the option while the call ran"
    assert torch.equal(c.fwd(), base[1])  # the default again


def test_generation_bumps_from_another_thread_recapture_mid_run(golden_dir):
    """the ImageNet tiny with "graph" 1 for itself runs on a worker; the main thread changes a process default its shapes never consult
    ("attn_tail_split": the head_dim-96 kernel's; this model has 48) once per four calls of the worker, while the next call runs.  Every
    change moves lt_opt_generation, a part of the graph key: the engine goes eager, captures and replays again, mid-run, several times.
    Outputs stay on the baseline and graph_replays() never decreases."""
    c = _Case(golden_dir, "imagenet")
    c.engine.set_option("graph", 1)
    base = c.baselines()
    calls, per_flip = 24, 4
    progress = threading.Semaphore(0)
    replays, outs = [c.engine.graph_replays()], []

    def worker():
        try:
            for i in range(calls):
                outs.append(c.call(i))
                replays.append(c.engine.graph_replays())
                progress.release()
        finally:
            for _ in range(calls):  # (a failed worker must not leave the main thread waiting)
                progress.release()

    def bumper():
        for k in range(calls // per_flip - 1):
            for _ in range(per_flip):
                assert progress.acquire(timeout=JOIN_TIMEOUT)
            set_option("attn_tail_split", 3 + (k & 1))

    try:
        _run_workers([worker], bumper)
    finally:
        set_option("attn_tail_split", 4)
    assert len(outs) == calls
    for i, o in enumerate(outs):
        assert torch.equal(o, base[i % 2]), f"call {i} left its baseline after a generation bump from the main thread"
    assert replays == sorted(replays) and replays[-1] > replays[0], replays
    print(f"graph_replays after each call: {replays}")
    assert torch.equal(c.fwd(), base[0])


def test_one_engine_called_from_three_threads_in_turn(golden_dir):
    """"from any thread": one engine with "graph" 1 is called from thread 1 (eager run, capture, replay), after the join from thread 2 (replays
    what thread 1 captured), then from the main thread.  Equal outputs, and the main thread's option scope, stream and device are its own
    again afterwards."""
    c = _Case(golden_dir, "next")
    c.engine.set_option("graph", 1)
    base = c.baselines()
    _new_generation(c.engine)
    got = {}

    def on(name):
        def work():
            got[name] = [c.call(i) for i in range(4)]
        return work

    r0 = c.engine.graph_replays()
    _run_workers([on("thread 1")])
    r1 = c.engine.graph_replays()
    _run_workers([on("thread 2")])
    r2 = c.engine.graph_replays()
    on("main")()
    assert r1 > r0 and r2 > r1 and c.engine.graph_replays() > r2
    for name, outs in got.items():
        for i, o in enumerate(outs):
            assert torch.equal(o, base[i % 2]), (name, i)
    assert torch.cuda.current_stream() == torch.cuda.default_stream() and torch.cuda.current_device() == c.z.device.index
    v = C.c_int32(-1)  # no scope of the engine's leaked to this thread: the process default reads as the process default
    ok(lib().lt_engine_get_option(None, b"graph", C.byref(v)))
    assert v.value == 2 and c.engine.get_option("graph") == 1
