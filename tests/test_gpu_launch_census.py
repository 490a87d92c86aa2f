"""-m gpu: the launch census of one model evaluation per route of the transformer block.

The block's routes are bit-identical by design (tests/test_gpu_variants.py, test_gpu_packed_onewave.py and others compare their words), so
no comparison of outputs can tell that an evaluation took another route than it used to.  The engine's profile can: per kernel class
(0 GEMM, 1 attention, 2 other) it counts the launch brackets of an eager evaluation and sums the flops of the launches' shapes.  Every
configuration of scripts/launch_census.py - small-fused attention, one q / k / V launch below 2048 rows, the q / k pair kernel from 2048
rows, the fused QKV launch with raw queries and the pair layout at 8192 rows of the 2B width and each of those switched off, Flag-DiT,
the three MoE families, packed batches, a regional prompt, a layer-skip set, the parts of a step-cached evaluation - must give the counts,
the flops, `last_pair` and `layout_flips` of the table profiles/run_forward_split/launch_census.json, which that script recorded from
the commit before run_forward was split into stages and has to be recorded again only when a change means to move a launch."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("launch_census", os.path.join(REPO, "scripts", "launch_census.py"))
LC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LC)

with open(LC.TABLE) as _f:
    WANT = json.load(_f)["configs"]


@pytest.mark.parametrize("group", sorted(LC.GROUPS))
def test_launch_census_equals_the_recorded_table(group):
    got, want = LC.census(group), WANT[group]
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    bad = {}
    for name, row in got.items():
        w = want[name]
        same = row["launches"] == w["launches"] and row["last_pair"] == w["last_pair"] and row.get("layout_flips") == w.get("layout_flips")
        same = same and all(abs(a - b) <= 1e-9 * max(abs(b), 1.0) for a, b in zip(row["flops"], w["flops"]))
        if not same:
            bad[name] = {"got": row, "want": w}
    assert not bad, bad
