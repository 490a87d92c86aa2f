"""CPU: the helpers of the engine state tests (tests/engine_sequences.py) - the Eulerian circuit, the host model of the graph cache's FIFO
rule, the shape of the catalogues, and the loud entry's state under the torch reference model."""
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import models
from lumina_t2x_amd.engine import DiTEngine
from oracle import nextdit_oracle as O

import engine_sequences as ES

MODEL_CLASSES = {"next": models.NextDiT, "imagenet": models.imagenet.DiT_Llama, "flag": models.flag_dit.DiT_Llama, "moe": models.moe.DiT_Llama}


@pytest.mark.parametrize("n", [1, 2, 7, 25])
def test_circuit_visits_every_ordered_pair_exactly_once_and_returns(n):
    c = ES.circuit(n)
    assert len(c) == n * n + 1 and c[0] == c[-1] == 0 and set(c) == set(range(n))
    pairs = list(zip(c, c[1:]))
    assert len(set(pairs)) == len(pairs) == n * n  # n^2 distinct adjacent pairs out of n^2 possible: each exactly once, (a, a) included
    assert ES.circuit(n) == c  # a pure function


def test_fifo_replays_on_hand_worked_sequences():
    assert ES.fifo_replays([]) == 0
    assert ES.fifo_replays(["a"]) == 0 and ES.fifo_replays(["a", "a"]) == 1 and ES.fifo_replays(["a", "b", "a", "a"]) == 2
    # 16 keys cycled three times: the first lap runs eagerly, the other two replay
    assert ES.fifo_replays(list(range(16)) * 3) == 32
    # 17 keys cycled three times: key k is dropped one step before it comes round again, so every use is a first use
    assert ES.fifo_replays(list(range(17)) * 3) == 0
    # a key re-entering after eviction starts over: 0 is used twice (one replay), 16 more keys push it out, then it runs eagerly and replays
    assert ES.fifo_replays([0, 0] + list(range(1, 17)) + [0]) == 1
    assert ES.fifo_replays([0, 0] + list(range(1, 17)) + [0, 0]) == 2
    # the FIFO drops by age, not by use: 0 is used in between and is dropped all the same
    assert ES.fifo_replays(list(range(16)) + [0, 16, 0]) == 1
    # cap 2: a b a(replay) c(drops a) then b replays, or a starts over
    assert ES.fifo_replays(["a", "b", "a", "c", "b"], cap=2) == 2 and ES.fifo_replays(["a", "b", "a", "c", "a"], cap=2) == 1


@pytest.mark.parametrize("family", list(ES.CATALOGUES))
def test_catalogues_name_existing_methods_have_unique_names_and_cover_both_sizes(family):
    cat = ES.CATALOGUES[family]
    names = [e.name for e in cat]
    assert len(set(names)) == len(names)
    for e in cat:
        assert e.methods, e.name
        for m in e.methods:
            assert hasattr(MODEL_CLASSES[family], m) or hasattr(DiTEngine, m), (e.name, m)
        assert e.prompt in ("A", "A2", "B", "P4") and e.rule in ("t2i", "anagram"), e.name
    assert {16, 48} <= {e.size for e in cat}
    assert any(e.methods == ("forward",) for e in cat) and any("forward_with_cfg" in e.methods for e in cat)  # unguided and guided
    if family == "next":
        assert ES.distinct_keys(cat) >= 20  # the cache holds 16: the walk evicts, with a margin
        assert sum(e.needs is not None for e in cat) == 4 and sum(e.size == 0 for e in cat) == 4
    else:
        assert 6 <= len(cat) <= 8


def test_the_loud_entry_is_finite_under_the_torch_reference_model(golden_dir):
    from test_gpu_slg import _deep
    cfg, sd, cond = _deep(golden_dir, "next", device="cpu")
    I = ES.Inputs("next", cond, device="cpu")
    z = I.z[48] * float(2 ** ES.LOUD_EXP)
    assert float(z.float().abs().max()) > 2.0 ** (ES.LOUD_EXP - 1) and bool(torch.isfinite(z.float()).all())
    cap, mask = I.cond()
    out = O.forward_with_cfg(sd, cfg, z.float(), I.t, cap.float(), mask, 4.0, **ES.STEP_KW)
    assert out.shape == z.shape and bool(torch.isfinite(out).all())
    assert bool(torch.isfinite(out.to(torch.bfloat16).float()).all())  # ... and in the engine's output format
