"""The exact-softmax attention tier without a GPU: both input families meet their preconditions and the ambiguity cap at every shape class
tests/test_gpu_attention_exact.py draws; a plain fp32 tile-by-tile emulation of the flash recurrence (64-key tiles, deferred maximum with
THR 8, bf16 P, row sum from the bf16 or the fp32 P) passes the comparator - a correct kernel alone stays inside the criterion - and every
planted local fault makes it fire, including the ones the global rel-L2 gate of tests/test_gpu_ops.py lets through."""
import math

import pytest
import torch

import exact_attention as X
from exact_operands import PreconditionError

INF = float("inf")
THR = 8.0


# ---- the emulation -----------------------------------------------------------------------------------------------------------------------
def _exp2(x):
    return torch.exp2(x.double()).float()   # exact at integers on any host libm


def flash(q, kbuf, vt, Nk, bias=None, rowsum="bf16", fault=None, tiles=None):
    """unnormalised (O, m, l) of one head in fp32: q [N, hd], kbuf [Nkpad, hd] (rows >= Nk: whatever lies behind the keys), vt [hd, Nkpad] in
    the V^T layout (keys >= Nk zero), bias [Nkpad] or None; `tiles`: the 64-key tiles to run (a tail-split part), default all"""
    f = fault or {}
    N, hd = q.shape
    rows = torch.arange(N)
    m, l, O = torch.full((N,), -INF), torch.zeros(N), torch.zeros(N, hd)
    for t in (range(vt.shape[1] // 64) if tiles is None else tiles):
        if f.get("skip_tile") == t:
            continue
        j = torch.arange(64 * t, 64 * t + 64)
        s = q @ kbuf[j].t()
        if not f.get("no_tail_mask"):
            s[:, j >= Nk] = -INF
        if bias is not None:
            s = s + bias[j][None, :]
        if "drop_key" in f and f["drop_key"][1] // 64 == t:
            s[rows // 256 == f["drop_key"][0], f["drop_key"][1] % 64] = -INF
        if "drop_tile" in f and f["drop_tile"][1] == t:
            s[rows // 256 == f["drop_tile"][0]] = -INF
        mx = s.max(1).values
        raise_ = mx > m + THR                                   # (m = -inf: the first tile with a finite score sets the maximum)
        m_new = torch.where(raise_, mx, m)
        alpha = torch.where(torch.isinf(m), torch.ones(N), _exp2(m - m_new))
        if f.get("skip_rescale"):
            alpha = torch.ones(N)
        O, l, m = O * alpha[:, None], l * alpha, m_new
        P = torch.where(torch.isinf(s) | torch.isinf(m)[:, None], torch.zeros_like(s), _exp2(s - m[:, None] - f.get("frac_max", 0.0)))
        Pb = P.to(torch.bfloat16).float()
        l = l + (P if rowsum == "fp32" or f.get("sum_unrounded") else Pb).sum(1)
        O = O + Pb @ vt[:, j if f.get("no_vperm") else X.v_position(j)].t()
    return O, m, l


def finish(O, l):
    return (O * (1.0 / l)[:, None]).to(torch.bfloat16)


def merge(parts, twice=None):
    """the tail split's merge of (O, m, l) partials over disjoint key ranges; twice: index of a part that is (wrongly) added again"""
    parts = list(parts) + ([parts[twice]] if twice is not None else [])
    M = torch.stack([p[1] for p in parts]).max(0).values
    w = [_exp2(p[1] - M) for p in parts]
    return finish(sum(wi[:, None] * p[0] for wi, p in zip(w, parts)), sum(wi * p[2] for wi, p in zip(w, parts)))


def emulate(inp, rowsum="bf16", use_bias=False, fault=None, at=(0, 0), kv_shift=0, split=None, twice=None):
    """bf16 [B, H, N, hd]: flash() on every head; `fault` is planted in head `at` only; kv_shift: that head reads kv-head (kvh + shift);
    split = number of tail-split parts for the rows of the last (partial) 256-row block"""
    q, k, v = inp["q"].float(), inp["k"].float(), inp["v"].float()
    B, H, N, hd = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    Nkpad, rep = X.pad64(Nk), H // Hkv
    vt = X.make_vt(v, Nkpad)
    bias = X.make_bias(inp["valid"], Nk, Nkpad, "cpu") if use_bias else None
    out = torch.empty(B, H, N, hd, dtype=torch.bfloat16)
    for b in range(B):
        for h in range(H):
            hit = (b, h) == tuple(at)
            kvh = (h // rep + (kv_shift if hit else 0)) % Hkv
            kbuf = k[b, kvh][torch.arange(Nkpad) % Nk]                          # a kernel that reads past Nk finds other keys there
            args = (kbuf, vt[b, kvh], Nk, None if bias is None else bias[b], rowsum, fault if hit else None)
            O, m, l = flash(q[b, h], *args)
            out[b, h] = finish(O, l)
            if split and N % 256:
                r0, nt = N // 256 * 256, Nkpad // 64
                cuts = [nt * s // split for s in range(split + 1)]
                parts = [flash(q[b, h, r0:], *args, tiles=range(cuts[s], cuts[s + 1])) for s in range(split)]
                out[b, h, r0:] = merge(parts, twice if hit else None)
    return out


def emulate_fused(a, t, gate, rowsum="bf16", fault=None, at=(0, 0), drop_gate=False):
    o_self = emulate(a, rowsum).float()
    o_txt = emulate(t, rowsum, use_bias=True, fault=fault, at=at).float()
    gt = X._r16(torch.tanh(gate.float())).view(1, -1, 1, 1)
    if drop_gate:
        gt = torch.ones_like(gt)
    return X._r16(o_self + X._r16(o_txt * gt)).to(torch.bfloat16)


# ---- the inputs meet their preconditions -------------------------------------------------------------------------------------------------
# one CPU-sized shape per class of the GPU file: ragged, every remainder of the unrolled loop, long, GQA 1 and 4, every head dim
SELF_SHAPES = [(2, 4, 1, 200, 72), (1, 4, 4, 40, 48), (1, 4, 4, 64, 128), (1, 2, 2, 321, 96), (1, 1, 1, 1000, 128), (1, 4, 4, 128, 48), (1, 4, 1, 192, 72),
               (2, 2, 2, 320, 96), (1, 1, 1, 384, 128), (1, 2, 1, 448, 72), (1, 2, 2, 1024, 48), (1, 1, 1, 2112, 96), (1, 1, 1, 4160, 96)]


@pytest.mark.parametrize("family", X.GENERATORS)
@pytest.mark.parametrize("B,H,Hkv,N,hd", SELF_SHAPES)
def test_self_attention_inputs_meet_the_preconditions(B, H, Hkv, N, hd, family):
    inp = X.GENERATORS[family](B, H, Hkv, N, N, hd, seed=N + hd)
    x = X.expected(inp)   # raises PreconditionError on any violation
    assert float(X.neighbours(x)[3].double().mean()) <= X.MAX_AMBIGUOUS
    st = inp["stats"]
    if family == "selector":
        assert st["min_live"] == st["max_live"] == 1
        assert len(torch.unique(inp["sel"][0, 0])) == N                      # a different key for every row
        if H > 1:
            assert not torch.equal(inp["sel"][0, 0], inp["sel"][0, 1])
    else:
        assert X.every_reduction_index_is_used(inp)
        assert st["max_live"] <= 2100 and st["min_live"] >= 1
        if N > 64:   # both the jump over THR and the rise below it occur
            assert st["jump"] > 0 and st["small_raise"] > 0, st
        # live keys on the first and the last key of every tile and on the last key, for every row class that keeps the tile
        s = inp["q"][0, 0].double() @ inp["k"][0, 0].double().t()
        live = (s - s.max(1, keepdim=True).values) >= -7
        edge = torch.tensor(sorted({j for j in range(N) if j % 64 in (0, 63)} | {N - 1}))
        assert bool(live[:, edge].any(0).all()) and bool(live[:, N - 1].any())


def test_the_long_case_meets_the_preconditions():
    """12800 keys (attn_fwd_kernel_v4<72>'s long case), the first 512 rows' worth of checks via a 512-query draw over all keys"""
    for family in X.GENERATORS:
        inp = X.GENERATORS[family](1, 1, 1, 512, 12800, 72, seed=5)
        x = X.expected(inp, row_chunk=256)
        assert float(X.neighbours(x)[3].double().mean()) <= X.MAX_AMBIGUOUS
        assert float(X.neighbours(x, 2.0 ** -14)[3].double().mean()) <= X.MAX_AMBIGUOUS   # the cap holds up to the widest DELTA allowed


@pytest.mark.parametrize("family", X.GENERATORS)
@pytest.mark.parametrize("hd", [48, 72, 96, 128])
@pytest.mark.parametrize("T,valid1", [(13, 5), (16, 8), (77, 77), (128, 8), (200, 130)])
def test_text_inputs_with_accumulate_meet_the_preconditions(T, valid1, hd, family):
    B, H, Hkv, N = 2, 6, 2, 96
    inp = X.GENERATORS[family](B, H, Hkv, N, T, hd, seed=T + hd, valid=(T, valid1))
    x = X.expected(inp)
    gate, prev = X.gate_values(H, T), X.small_int_prev(B, H, N, hd, T)
    assert sorted(set(X._r16(torch.tanh(gate.float())).tolist())) == [-1.0, 0.0, 1.0]
    want, cands, amb = X.admissible([x], X.gated(prev, gate))
    assert float(amb.double().mean()) <= X.MAX_AMBIGUOUS and len(cands) == 3
    assert torch.equal(want, X._r16(want))


@pytest.mark.parametrize("family", X.GENERATORS)
@pytest.mark.parametrize("hd", [72, 96])
@pytest.mark.parametrize("B,H,Hkv,N,T,valid", [(2, 6, 2, 320, 128, (128, 8)), (2, 3, 3, 192, 77, (77, 1)), (2, 6, 2, 256, 200, (60, 130)),
                                                (2, 3, 1, 128, 64, (64, 33)), (2, 6, 6, 128, 300, (300, 130))])
def test_fused_inputs_meet_the_preconditions_with_one_query_tensor(B, H, Hkv, N, T, valid, hd, family):
    a, t = X.fused_draw(family, B, H, Hkv, N, T, hd, N + T + hd, valid, "cpu")
    assert a["q"] is t["q"]
    xs, xt = X.expected(a), X.expected(t)
    _, cands, amb = X.admissible([xs, xt], X.fused(X.gate_values(H, T)))
    assert float(amb.double().mean()) <= X.MAX_AMBIGUOUS and len(cands) == 9


def test_expected_refuses_inputs_that_are_not_exact():
    inp = X.levels(1, 2, 1, 128, 128, 72, seed=1)
    with pytest.raises(PreconditionError, match="k_prescaled"):
        X.expected(inp, k_prescaled=0, scale=0.1)
    bad = dict(inp, q=(inp["q"].float() * 0.5).to(torch.bfloat16))
    with pytest.raises(PreconditionError, match="integers"):
        X.expected(bad)
    bad = dict(inp, k=inp["k"].clone())
    bad["k"][0, 0, 5] = inp["k"][0, 0, 5] * 4                                 # a key 20-odd below the maximum: neither a level nor off
    with pytest.raises(PreconditionError):
        X.expected(bad)
    bad = dict(inp, v=(inp["v"].float().abs() * 32 + 32).to(torch.bfloat16))  # sum_live 2^level |v| far above 512
    with pytest.raises(PreconditionError, match="512"):
        X.expected(bad)
    sel = X.selector(1, 2, 1, 128, 128, 72, seed=1)
    bad = dict(sel, k=sel["k"].clone())
    bad["k"][0, 0, 7] = sel["k"][0, 0, 8]                                      # two keys with one code: rows selecting 8 see two live keys
    with pytest.raises(PreconditionError, match="selector"):
        X.expected(bad)
    x = torch.tensor([[[[1.0 + 2.0 ** -8, 3.0, 0.0, -(1.0 + 3 * 2.0 ** -8 + 2.0 ** -30)]]]], dtype=torch.float64)
    rn, lo, hi, amb = X.neighbours(x)
    assert rn.flatten().tolist() == [1.0, 3.0, 0.0, -(1.0 + 2.0 ** -6)] and amb.flatten().tolist() == [True, False, False, True]   # ties to even
    assert lo.flatten().tolist()[0] == 1.0 and hi.flatten().tolist()[0] == 1.0 + 2.0 ** -7
    with pytest.raises(PreconditionError, match="midpoint"):
        X.assert_attention_words(torch.ones(1, 1, 1, 4).bfloat16(), [x.expand(1, 1, 1, 4) * 0 + 1.0 + 2.0 ** -8])


# ---- a correct recurrence passes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rowsum", ["bf16", "fp32"])
@pytest.mark.parametrize("family", X.GENERATORS)
@pytest.mark.parametrize("B,H,Hkv,N,hd", [(2, 4, 1, 200, 72), (1, 2, 2, 321, 96), (1, 2, 1, 448, 48), (1, 1, 1, 1000, 128), (1, 2, 2, 1024, 72)])
def test_the_emulated_recurrence_passes_the_comparator(B, H, Hkv, N, hd, family, rowsum):
    inp = X.GENERATORS[family](B, H, Hkv, N, N, hd, seed=N + hd)
    X.assert_attention_words(emulate(inp, rowsum), [X.expected(inp)], what="emulation", inp=inp)


@pytest.mark.parametrize("rowsum", ["bf16", "fp32"])
@pytest.mark.parametrize("family", X.GENERATORS)
def test_the_emulated_text_fused_and_split_forms_pass_the_comparator(family, rowsum):
    B, H, Hkv, N, hd = 2, 6, 2, 96, 72
    for T, valid1 in [(13, 5), (77, 77), (200, 130)]:
        inp = X.GENERATORS[family](B, H, Hkv, N, T, hd, seed=T + hd, valid=(T, valid1))
        gate, prev = X.gate_values(H, T), X.small_int_prev(B, H, N, hd, T)
        got = X.gated(prev, gate)(emulate(inp, rowsum, use_bias=True).float()).to(torch.bfloat16)
        X.assert_attention_words(got, [X.expected(inp)], X.gated(prev, gate), what="emulated accumulate")
    a, t = X.fused_draw(family, 2, 3, 3, 192, 200, 96, 7, (130, 1), "cpu")
    gate = X.gate_values(3, 1)
    X.assert_attention_words(emulate_fused(a, t, gate, rowsum), [X.expected(a), X.expected(t)], X.fused(gate), what="emulated fused")
    inp = X.GENERATORS[family](1, 2, 1, 1088, 1088, 96, seed=3)
    for parts in (2, 3, 4):
        X.assert_attention_words(emulate(inp, rowsum, split=parts), [X.expected(inp)], what=f"emulated tail split {parts}", inp=inp)


# ---- planted faults ----------------------------------------------------------------------------------------------------------------------
def _self_inputs(family="levels"):
    return X.GENERATORS[family](2, 4, 2, 576, 576, 72, seed=11)   # 9 tiles, three 256-row blocks (the last of 64 rows), GQA 2


SELF_FAULTS = {
    "one key dropped in one q-block": dict(fault={"drop_key": (1, 3 * 64)}),
    "tile dropped, tiles % 4 == 0": dict(fault={"drop_tile": (0, 4)}),
    "tile dropped, tiles % 4 == 1": dict(fault={"drop_tile": (1, 5)}),
    "tile dropped, tiles % 4 == 2": dict(fault={"drop_tile": (1, 2)}),
    "tile dropped, tiles % 4 == 3": dict(fault={"drop_tile": (0, 7)}),
    "V^T key permutation ignored": dict(fault={"no_vperm": True}),
    "GQA head reads the neighbouring kv-head": dict(kv_shift=1),
    "rescale skipped after a jump over THR": dict(fault={"skip_rescale": True}),
    "row sum from the unrounded P at a level where it differs from the bf16 P": dict(fault={"frac_max": 0.3, "sum_unrounded": True}),
}


LEVELS_ONLY = ("row sum from the unrounded P at a level where it differs from the bf16 P",)   # one live key: O and l move together


@pytest.mark.parametrize("name,family", [(n, f) for n in SELF_FAULTS for f in X.GENERATORS if not (f == "selector" and n in LEVELS_ONLY)])
def test_planted_self_attention_faults_are_caught(name, family):
    """each fault sits in ONE head (b 1, h 2) - the q-block faults in one 256-row block of it; the comparator names that head.  (The row-sum
    fault: with integer scores every P is a power of two and its bf16 rounding is the identity, so the fault is planted together with a
    running maximum that is off by a fraction - the only way P and bf16(P) can differ - and PV then multiplies another P than l adds.)"""
    inp = _self_inputs(family)
    kw = dict(SELF_FAULTS[name])
    if family == "selector" and "drop_key" in kw.get("fault", {}):   # the key row 300 of this head selects
        kw["fault"] = {"drop_key": (1, int(inp["sel"][1, 2, 300]))}
    with pytest.raises(AssertionError, match=r"largest: \(b 1, h 2,") as e:
        X.assert_attention_words(emulate(inp, at=(1, 2), **kw), [X.expected(inp)], what=name, inp=inp)
    if "q-block" in name:
        assert "rows 256-" in str(e.value) or "rows 320-" in str(e.value) or "rows 384-" in str(e.value) or "rows 448-" in str(e.value)


@pytest.mark.parametrize("family", X.GENERATORS)
def test_unmasked_tail_keys_are_caught(family):
    inp = X.GENERATORS[family](1, 2, 2, 200, 200, 72, seed=2)   # 200 keys: 56 positions of the last tile lie behind the keys
    with pytest.raises(AssertionError, match="words wrong"):
        X.assert_attention_words(emulate(inp, fault={"no_tail_mask": True}, at=(0, 1)), [X.expected(inp)], what="tail", inp=inp)


@pytest.mark.parametrize("name,family", [("one masked text key counted", "levels"),   # (no selector row selects a masked key)
                                         ("a text tile skipped that holds a valid key", "levels"), ("a text tile skipped that holds a valid key", "selector"),
                                         ("the gate dropped", "levels"), ("the gate dropped", "selector")])
def test_planted_text_faults_are_caught(name, family):
    B, H, Hkv, N, T, hd = 2, 3, 3, 128, 200, 72
    a, t = X.fused_draw(family, B, H, Hkv, N, T, hd, 5, (200, 130), "cpu")
    gate = X.gate_values(H, 0)   # +1, -1, 0 on heads 0, 1, 2
    if name == "one masked text key counted":   # key 192 of sample 1 (valid 130): the first key of a tile, live for the rows that keep its class
        got_t = emulate(t, use_bias=True).float()
        bias = X.make_bias(t["valid"], T, X.pad64(T), "cpu")
        bias[1, 192] = 0.0
        q, kk, vt = t["q"].float(), t["k"].float(), X.make_vt(t["v"].float(), X.pad64(T))
        O, m, l = flash(q[1, 1], kk[1, 1][torch.arange(X.pad64(T)) % T], vt[1, 1], T, bias[1])
        got_t[1, 1] = finish(O, l).float()
        gt = X._r16(torch.tanh(gate.float())).view(1, -1, 1, 1)
        got = X._r16(emulate(a).float() + X._r16(got_t * gt)).to(torch.bfloat16)
    elif name == "a text tile skipped that holds a valid key":   # tile 2 of sample 1 holds its last two valid keys (128, 129)
        got = emulate_fused(a, t, gate, fault={"skip_tile": 2}, at=(1, 1))
    else:
        got = emulate_fused(a, t, gate, drop_gate=True)
    with pytest.raises(AssertionError, match="words wrong") as e:
        X.assert_attention_words(got, [X.expected(a), X.expected(t)], X.fused(gate), what=name)
    if name != "the gate dropped":
        assert "largest: (b 1, h 1," in str(e.value)
    else:
        assert "h 0," not in str(e.value).split("first:")[0]   # tanh(+20) = 1: head 0 is right with or without its gate


@pytest.mark.parametrize("parts,twice", [(2, 1), (4, 0), (3, 2)])
def test_a_tail_split_part_merged_twice_is_caught(parts, twice):
    """(levels only: with one live key a part counted twice doubles O and l alike)"""
    inp = X.levels(1, 2, 1, 1088, 1088, 96, seed=3)   # 4 x 256 + 64 rows
    with pytest.raises(AssertionError, match=r"largest: \(b 0, h 1, rows 1024-1087") as e:
        X.assert_attention_words(emulate(inp, split=parts, twice=twice, at=(0, 1)), [X.expected(inp)], what="merge", inp=inp)
    assert "rows 0-" not in str(e.value)


def test_a_wrong_selector_word_names_its_source():
    inp = X.selector(1, 4, 2, 128, 128, 72, seed=4)
    x = X.expected(inp)
    got = x.to(torch.bfloat16)
    got[0, 3, 17, 5] = inp["v"][0, 0, 99, 5]   # head 3 (kv-head 1), row 17 holds key 99 of kv-head 0
    with pytest.raises(AssertionError, match=r"\(kvh 0, key 99\)"):
        X.assert_attention_words(got, [x], what="source", inp=inp)
    got = x.to(torch.bfloat16)
    got[0, 0, 64:128] = float("nan")
    with pytest.raises(AssertionError, match=r"4608 of \d+ words wrong \(4608 unwritten"):
        X.assert_attention_words(got, [x], what="unwritten", inp=inp)


# ---- the global rel-L2 gate does not see them ---------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_the_global_rel_l2_gate_misses_the_one_q_block_faults():
    """test_attention_self's criterion (randn inputs, its entropy scale, rel_l2 < 6e-3 over the whole output) on the same emulation with
    the same faults in ONE 256-row block, at (2, 8, 8, 1024) hd 72 - the (2, 32, 32, 4096) case scaled down to what a CPU run affords:
    2 x 8 x 4 = 64 blocks instead of 1024, a tile 1/16 of the keys instead of 1/64.  Measured here (whole output | the faulty block alone):
        no fault (bf16 rounding of P and of the output)   3.29e-3
        one key dropped in one q-block                     5.04e-3 | 3.15e-2   -> passes the 6e-3 gate already at 64 blocks
        one tile dropped in one q-block                    3.06e-2 | 2.49e-1   -> seen at 64 blocks with 16 tiles; the block-alone error of a
                                                                                  tile at 64 tiles is 1.3e-1, over 1024 blocks 1.3e-1 / 32 = 4e-3
    The key fault's block-alone error over the GPU case's 1024 blocks is 3.15e-2 / 32 = 1e-3, below the rounding floor.  The exact
    comparator fires on both faults at this very shape, and names the block."""
    B, H, N, hd = 2, 8, 1024, 72
    g = torch.Generator().manual_seed(N + hd)
    q, k, v = (torch.randn(B, H, N, hd, generator=g).to(torch.bfloat16) for _ in range(3))
    scale = math.sqrt(math.log(N, 64) / hd)
    kf = (k.float() * (scale * X.L2E)).to(torch.bfloat16)
    ref = torch.softmax((q.double() @ k.double().transpose(2, 3)) * scale, -1) @ v.double()
    rnd = dict(family="randn", q=q, k=kf, v=v, valid=[N] * B)
    clean = _rel_l2(emulate(rnd), ref)
    exact = X.levels(B, H, H, N, N, hd, seed=1)
    want = X.expected(exact)
    figures = {}
    for name, fault, efault in (("key", {"drop_key": (2, 517)}, {"drop_key": (2, 512)}), ("tile", {"drop_tile": (2, 9)}, {"drop_tile": (2, 9)})):
        got = emulate(rnd, fault=fault, at=(1, 3))
        figures[name] = (_rel_l2(got, ref), _rel_l2(got[1, 3, 512:768], ref[1, 3, 512:768]))
        with pytest.raises(AssertionError, match=r"largest: \(b 1, h 3, rows (512|576|640|704)-"):
            X.assert_attention_words(emulate(exact, fault=efault, at=(1, 3)), [want], what=name)
    print(f"rel-L2: clean {clean:.2e}, key dropped {figures['key']}, tile dropped {figures['tile']}")
    assert clean < 6e-3
    assert figures["key"][0] < 6e-3 < figures["key"][1]                      # the gate passes the output; the block alone is far out
    assert figures["key"][1] / 32 < clean and figures["tile"][1] > 6e-3      # ... and over 1024 blocks it sinks below the rounding floor
