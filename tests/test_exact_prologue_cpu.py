"""CPU: every case of tests/test_gpu_prologue_exact.py, without the kernels (tests/exact_prologue.py).  Per case: an fp32 restatement of the
prologue (torch fp32, plain and with the contracted multiply-add) turns the raw buffers into the integer targets bit for bit; every word is
determined (cap 0); the generator's preconditions and the ambiguity cap hold; the rotation convention is the oracle's.  Then the planted
faults: each one, applied to the restatement of ONE head, must fail the comparator, and the message must name that head."""
import functools
import re

import pytest
import torch

import exact_attention as X
import exact_prologue as E

FAMILIES = ["selector", "levels"]


_seed = E.case_seed


@functools.lru_cache(maxsize=None)
def _qraw_case(family, shape):
    B, H, Hkv, N, grid_w = shape
    inp = E.draw(family, B, H, Hkv, N, 72, _seed(*shape))
    return inp, X.expected(inp)


@functools.lru_cache(maxsize=None)
def _small_case(family, shape):
    B, N, H, Hkv, grid_w = shape
    inp = E.draw(family, B, H, Hkv, N, 48, _seed(*shape))
    return inp, X.expected(inp)


def _same_words(a, b):
    return torch.equal(a.float(), b.float())   # (-0 == 0: a signed swap of a zero may carry the sign)


def test_the_table_is_quarter_turns_and_the_branches_differ_everywhere():
    table, table_t = E.quarter_turn_table(2, 70, 72, 5)
    assert table.shape == (2, 70, 18, 2) and table_t.shape == (2, 18, 70, 2) and torch.equal(table_t, table.permute(0, 2, 1, 3))
    assert bool(((table[..., 0].abs() + table[..., 1].abs()) == 1).all()) and set(table.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert bool((table[0] != table[1]).any(-1).all())
    for br in (0, 1):   # every quarter turn occurs, neighbouring frequencies and positions mostly differ
        qt = (table[br, ..., 0] == 1) * 0 + (table[br, ..., 1] == 1) * 1 + (table[br, ..., 0] == -1) * 2 + (table[br, ..., 1] == -1) * 3
        assert sorted(qt.unique().tolist()) == [0, 1, 2, 3]
        assert float((qt[:, 1:] != qt[:, :-1]).float().mean()) > 0.6 and float((qt[1:] != qt[:-1]).float().mean()) > 0.6


@pytest.mark.parametrize("grid_w", [8, 13])
@pytest.mark.parametrize("branch", [0, 1])
def test_unrotate_inverts_the_oracles_rotary_bit_for_bit(branch, grid_w):
    from oracle import nextdit_oracle as O
    B, H, N, hd = 2, 3, 104, 48
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), hd, 9)
    target = (X._mix(X._ar(B * H * N * hd, "cpu"), 3) % 257 - 128).float().view(B, H, N, hd)
    y = E.unrotate(target, table, branch, grid_w)
    # the oracle's layout: x [B, N, H, hd], freqs_cis [1, N, hd / 2] complex; slot pr = 2 f + axis (axis 0: row position, 1: column position)
    n = torch.arange(N)
    rows, cols = table[branch, n // grid_w], table[branch, n % grid_w]                       # [N, hd / 4, 2]
    cs = torch.stack([rows, cols], 2).reshape(N, hd // 2, 2)
    freqs = torch.view_as_complex(cs.contiguous()).unsqueeze(0)
    back = O.apply_rotary(y.permute(0, 2, 1, 3).contiguous(), freqs).permute(0, 2, 1, 3)
    assert torch.equal(back, target)
    for fma in (False, True):
        assert torch.equal(E.rotate(y, table, branch, grid_w, fma), target)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", E.QRAW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_qraw_cases_are_determined_and_restate_bit_for_bit(shape, family):
    B, H, Hkv, N, grid_w = shape
    inp, want = _qraw_case(family, shape)
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 72, _seed(*shape))
    assert table.shape[1] > grid_w and table.shape[1] > (N - 1) // grid_w + 1
    _, _, amb = X.admissible([want], lambda o: o)
    assert float(amb.double().mean()) <= X.MAX_AMBIGUOUS
    raws = {}
    for tname in E.QRAW_T:
        t = E.T_VALUE[tname]
        raw = raws[tname] = E.qraw_from_target(inp["q"], table, E.branch_of(t), grid_w, _seed(*shape))   # (raises unless every word is determined)
        assert bool(E.determined(raw["x"], raw["mean"], raw["rstd"], raw["wd"], raw["bd"], raw["yt"]).all())
        used = torch.zeros_like(raw["qkv"], dtype=torch.bool)
        used[:, raw["q_col0"]:raw["q_col0"] + H * 72] = True
        assert bool(torch.isnan(raw["qkv"].float())[~used].all()) and not bool(torch.isnan(raw["qkv"].float())[used].any())
        assert raw["q_col0"] > 0 and raw["ld"] > raw["q_col0"] + H * 72
        for fma in (False, True):
            assert _same_words(E.restate_qraw(raw, B, H, 72, t, fma), inp["q"]), (tname, fma)
    assert not torch.equal(raws["below"]["qkv"].view(torch.int16), raws["above"]["qkv"].view(torch.int16))   # the branch matters
    assert torch.equal(raws["null"]["qkv"].view(torch.int16), raws["above"]["qkv"].view(torch.int16))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape,T,valid,tname", E.QRAW_TEXT, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_qraw_text_cases_are_determined_and_restate_bit_for_bit(shape, T, valid, tname, family):
    B, H, Hkv, N, grid_w = shape
    assert B == 2 and len(valid) == 2
    a, t = E.draw_fused(family, B, H, Hkv, N, T, 72, _seed(*shape) + T, valid)
    want_self, want_txt = X.expected(a), X.expected(t)
    gate = X.gate_values(H, T)
    _, _, amb = X.admissible([want_self, want_txt], X.fused(gate))
    assert float(amb.double().mean()) <= X.MAX_AMBIGUOUS
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 72, _seed(*shape))
    tv = E.T_VALUE[tname]
    raw = E.qraw_from_target(a["q"], table, E.branch_of(tv), grid_w, _seed(*shape) + T)
    for fma in (False, True):
        assert _same_words(E.restate_qraw(raw, B, H, 72, tv, fma), a["q"])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", E.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_small_cases_are_determined_and_restate_bit_for_bit(shape, family):
    B, N, H, Hkv, grid_w = shape
    inp, want = _small_case(family, shape)
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 48, _seed(*shape))
    _, _, amb = X.admissible([want], lambda o: o)
    assert float(amb.double().mean()) <= X.MAX_AMBIGUOUS
    for tname in ("below", "above"):
        t = E.T_VALUE[tname]
        for ks in E.K_SCALES:
            raw = E.small_from_target(inp["q"], inp["k"], inp["v"], table, E.branch_of(t), grid_w, ks, _seed(*shape))   # (raises unless determined)
            rs = raw["rowstat"].double()
            for s0, ns, W in ((raw["q_slot0"], raw["q_nslot"], H * 48), (raw["k_slot0"], raw["k_nslot"], Hkv * 48)):
                part = rs[:, s0:s0 + ns]
                assert bool((part[..., 0].sum(1) == 0).all()) and bool((part[..., 1].sum(1) == W * 4 ** E.J).all())
                assert bool((part == part.round()).all()) and bool((part[..., 1] > 0).all())
                for drop in (part[:, 1:], part[:, :-1]):       # one slot too few: the squares shrink by a factor >= 1.25, the mean moves
                    assert bool((drop[..., 1].sum(1) * 1.25 <= W * 4 ** E.J).all()) and bool((drop[..., 0].sum(1) != 0).all())
            owned = torch.zeros(raw["slots"], dtype=torch.bool)
            owned[raw["q_slot0"]:raw["q_slot0"] + raw["q_nslot"]] = owned[raw["k_slot0"]:raw["k_slot0"] + raw["k_nslot"]] = True
            assert bool((raw["rowstat"][:, ~owned] == E.POISON_STAT).all())
            assert raw["q_col0"] > 0 and float(torch.isnan(raw["qkv"].float()).sum()) == raw["qkv"].shape[0] * 32
            for fma in (False, True):
                q, k, v = E.restate_small(raw, t, fma)
                assert _same_words(q, inp["q"]) and _same_words(k, inp["k"]) and torch.equal(v, inp["v"]), (tname, ks, fma)


# ---- planted faults -------------------------------------------------------------------------------------------------------------------------
def _must_fail_on_head(got64, wants, combine, head, what):
    with pytest.raises(AssertionError) as err:
        X.assert_attention_words(got64.to(torch.bfloat16), wants, combine, what=what)
    msg = str(err.value)
    named = set(int(h) for h in re.findall(r"\(b \d+, h (\d+), row", msg))
    assert named == {head}, (what, head, msg)


# The levels family sees every fault: a score that moves by one unit moves a weight by a factor two.  The selector family decides by a margin
# of 256 between the selected key and every other; a fault that moves the scores by less (a bias or a rotary factor of one slot, a K scale of
# 1 / 2) cannot change its output by construction, so those pairs are not cases (every other fault must be caught by both families).
SELECTOR_BLIND = {("qraw", "freq"), ("qraw", "bias"), ("small", "bias"), ("small", "k_scale")}
QRAW_FAULTS = ["freq", "rowcol", "branch", "grid_w", "bias", "weight"]


def _fault_params(kernel, faults):
    return [(f, fam) for f in faults for fam in FAMILIES if not (fam == "selector" and (kernel, f) in SELECTOR_BLIND)]


@pytest.mark.parametrize("fault,family", _fault_params("qraw", QRAW_FAULTS))
def test_a_planted_fault_in_the_qraw_prologue_is_caught_and_located(fault, family):
    shape = E.QRAW_SHAPES[1]
    B, H, Hkv, N, grid_w = shape
    inp, want = _qraw_case(family, shape)
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 72, _seed(*shape))
    t = E.T_VALUE["below"]
    raw = E.qraw_from_target(inp["q"], table, E.branch_of(t), grid_w, _seed(*shape))
    clean = E.attention64(E.restate_qraw(raw, B, H, 72, t), inp["k"], inp["v"])
    X.assert_attention_words(clean.to(torch.bfloat16), [want], what="clean")
    head = 2
    q = E.restate_qraw(raw, B, H, 72, t, fault=fault, fault_head=head)
    _must_fail_on_head(E.attention64(q, inp["k"], inp["v"]), [want], lambda o: o, head, f"q_raw {fault}")


@pytest.mark.parametrize("family", FAMILIES)
def test_a_text_gate_taken_from_the_neighbouring_head_is_caught_and_located(family):
    shape, T, valid, _ = E.QRAW_TEXT[5]
    B, H, Hkv, N, grid_w = shape
    a, t = E.draw_fused(family, B, H, Hkv, N, T, 72, _seed(*shape) + T, valid)
    want_self, want_txt = X.expected(a), X.expected(t)
    gate = X.gate_values(H, T)
    o_self, o_txt = E.attention64(a["q"], a["k"], a["v"]), E.attention64(t["q"], t["k"], t["v"], t["valid"])
    got = X.fused(gate)(X._r16(o_self.float()), X._r16(o_txt.float()))
    X.assert_attention_words(got.to(torch.bfloat16), [want_self, want_txt], X.fused(gate), what="clean")
    head = 1
    wrong = gate.clone()
    wrong[head] = gate[(head + 1) % H]
    assert float(wrong[head]) != float(gate[head])
    got = X.fused(wrong)(X._r16(o_self.float()), X._r16(o_txt.float()))
    _must_fail_on_head(got.double(), [want_self, want_txt], X.fused(gate), head, "text gate of head + 1")


SMALL_FAULTS = ["freq", "rowcol", "branch", "grid_w", "bias", "weight", "kfreq", "krowcol", "kbranch", "kgrid_w", "kbias", "stat_drop", "stat_v", "k_scale", "v_keyperm", "v_swizzle"]


@pytest.mark.parametrize("fault,family", _fault_params("small", SMALL_FAULTS))
def test_a_planted_fault_in_the_small_kernels_prologue_is_caught_and_located(fault, family):
    shape = E.SMALL_SHAPES[1]
    B, N, H, Hkv, grid_w = shape
    inp, want = _small_case(family, shape)
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 48, _seed(*shape))
    t = E.T_VALUE["below"]
    raw = E.small_from_target(inp["q"], inp["k"], inp["v"], table, E.branch_of(t), grid_w, 2.0, _seed(*shape))
    X.assert_attention_words(E.attention64(*E.restate_small(raw, t)).to(torch.bfloat16), [want], what="clean")
    head = 5   # (H == Hkv at this shape: the faulty kv-head is seen by this query head alone)
    q, k, v = E.restate_small(raw, t, fault=fault, fault_head=head)
    _must_fail_on_head(E.attention64(q, k, v), [want], lambda o: o, head, f"small {fault}")
