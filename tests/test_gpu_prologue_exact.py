"""-m gpu: the two attention launches that build their operands themselves - AttnArgs::q_raw of attn_fwd_kernel_v4<72> (q_norm + 2-D RoPE from
the raw QKV rows) and attn_small_fused_kernel<48> (LayerNorm statistics from per-tile partials, q in registers, the k and V^T images in LDS) -
on raw operands from which the prologue must produce, bit for bit, the integer q / k of tests/exact_attention.py (tests/exact_prologue.py:
quarter-turn RoPE tables, power-of-two LayerNorm weights, chosen statistics; every prologue word determined, cap 0).  The expected value is
exact_attention.expected() on the generator's own q, k, v and the comparator assert_attention_words with DELTA and MAX_AMBIGUOUS unchanged:
every output word is the one correct word.  Both table branches are selected through t; the outputs are NaN-filled between sentinel guards
and every input is compared with its copy afterwards.  tests/test_exact_prologue_cpu.py checks the same cases without the kernels."""
import functools

import pytest
import torch

import exact_attention as X
import exact_operands as XO
import exact_prologue as E
from gpu_util import P, bf, lib, ok, set_option, stream

pytestmark = pytest.mark.gpu

FAMILIES = ["selector", "levels"]
QRAW_KERNEL = "attn_fwd_kernel_v4<72>"
SMALL_KERNEL = "attn_small_fused_kernel<48>"
_ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


@pytest.fixture(autouse=True)
def _default_options():
    yield
    set_option("attention_variant", 4)
    set_option("attn_text_skip", 1)


def _report(kernel, family, shape, share):
    print(f"PROLOGUE kernel={kernel} family={family} shape={shape} ambiguous={share:.4%} undetermined=0")


@functools.lru_cache(maxsize=2)
def _qraw_problem(family, shape):
    B, H, Hkv, N, grid_w = shape
    inp = E.draw(family, B, H, Hkv, N, 72, E.case_seed(*shape), device="cuda")
    return inp, X.expected(inp)


@functools.lru_cache(maxsize=2)
def _small_problem(family, shape):
    B, N, H, Hkv, grid_w = shape
    inp = E.draw(family, B, H, Hkv, N, 48, E.case_seed(*shape), device="cuda")
    return inp, X.expected(inp)


@pytest.mark.parametrize("tname", E.QRAW_T)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", E.QRAW_SHAPES, ids=_ids)
def test_qraw_prologue_is_word_exact(shape, family, tname):
    B, H, Hkv, N, grid_w = shape
    set_option("attention_variant", 4)
    assert X.describe(B, H, Hkv, N, N, 72) == QRAW_KERNEL
    inp, want = _qraw_problem(family, shape)
    t = E.T_VALUE[tname]
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 72, E.case_seed(*shape), "cuda")
    raw = E.qraw_from_target(inp["q"], table, E.branch_of(t), grid_w, E.case_seed(*shape))   # (raises unless every word is determined)
    what = f"{QRAW_KERNEL} q_raw {family} {shape} t {tname}"
    got = E.run_qraw(raw, inp, t, what=what)
    share = X.assert_attention_words(got, [want], what=what, inp=inp)
    _report(QRAW_KERNEL + "+q_raw", family, shape + (tname,), share)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape,T,valid,tname", E.QRAW_TEXT, ids=_ids)
def test_qraw_prologue_with_fused_text_is_word_exact(shape, T, valid, tname, family, skip):
    """the headline path: q from the prologue, the text keys in the same launch (two-slot draws; B = 2 with a short valid length on the second
    sample, on an MHA, an MQA and a GQA shape; the table branch through t)"""
    B, H, Hkv, N, grid_w = shape
    set_option("attention_variant", 4)
    set_option("attn_text_skip", skip)
    assert X.describe(B, H, Hkv, N, N, 72) == QRAW_KERNEL
    seed = E.case_seed(*shape)
    a, txt = E.draw_fused(family, B, H, Hkv, N, T, 72, seed + T, valid, "cuda")
    want_self, want_txt = X.expected(a), X.expected(txt)
    gate = X.gate_values(H, T, "cuda")
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 72, seed, "cuda")
    t = E.T_VALUE[tname]
    raw = E.qraw_from_target(a["q"], table, E.branch_of(t), grid_w, seed + T)
    what = f"{QRAW_KERNEL} q_raw + text {family} {shape} T {T} valid {valid} t {tname} text_skip {skip}"
    got = E.run_qraw(raw, a, t, txt=txt, gate=gate, what=what)
    share = X.assert_attention_words(got, [want_self, want_txt], X.fused(gate), what=what)
    _report(QRAW_KERNEL + "+q_raw+text", family, shape + (T, valid, tname, skip), share)


@pytest.mark.parametrize("k_scale", E.K_SCALES)
@pytest.mark.parametrize("tname", ["below", "above"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", E.SMALL_SHAPES, ids=_ids)
def test_small_fused_kernel_is_word_exact(shape, family, tname, k_scale):
    B, N, H, Hkv, grid_w = shape
    inp, want = _small_problem(family, shape)
    t = E.T_VALUE[tname]
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 48, E.case_seed(*shape), "cuda")
    raw = E.small_from_target(inp["q"], inp["k"], inp["v"], table, E.branch_of(t), grid_w, k_scale, E.case_seed(*shape))
    what = f"{SMALL_KERNEL} {family} {shape} t {tname} k_scale {k_scale}"
    got = E.run_small(raw, t, what=what)
    share = X.assert_attention_words(got, [want], what=what, inp=inp)
    _report(SMALL_KERNEL, family, shape + (tname, k_scale), share)


@pytest.mark.parametrize("why,override", [("tokens 96", dict(tokens=96)), ("tokens 576", dict(tokens=576)), ("head_dim 72", dict(hd=72)),
                                          ("k_nslot one too few", dict(k_nslot=-1)), ("grid_w larger than the table", dict(grid_w=0))])
def test_small_fused_kernel_refuses(why, override):
    """the entry returns non-zero and the guarded output stays NaN.  The buffers are those of a valid 2 x 128-token call: the test relies on
    launch_attention_small checking attention_small_fusable and its slot / table conditions before anything is launched (a launch with 576
    tokens would run past them)"""
    shape = E.SMALL_SHAPES[1]
    B, N, H, Hkv, grid_w = shape
    inp, _ = _small_problem("selector", shape)
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 48, E.case_seed(*shape), "cuda")
    raw = E.small_from_target(inp["q"], inp["k"], inp["v"], table, 1, grid_w, 1.0, E.case_seed(*shape))
    if "k_nslot" in override:
        override = dict(k_nslot=raw["k_nslot"] - 1)
    if "grid_w" in override:
        override = dict(grid_w=table.shape[1] + 1)
    E.run_small(raw, None, what=f"refusal: {why}", expect_refusal=True, **override)
    assert lib().lt_last_error()


def test_qraw_refuses_a_grid_larger_than_the_table():
    shape = E.QRAW_SHAPES[0]
    B, H, Hkv, N, grid_w = shape
    inp, _ = _qraw_problem("selector", shape)
    table, _ = E.quarter_turn_table(2, E.table_len(N, grid_w), 72, E.case_seed(*shape), "cuda")
    raw = E.qraw_from_target(inp["q"], table, 1, grid_w, E.case_seed(*shape))
    E.run_qraw(raw, inp, None, what="q_raw, grid_w > table", expect_refusal=True, grid_w=table.shape[1] + 1)
    E.run_qraw(raw, inp, None, what="q_raw, rows > table", expect_refusal=True, grid_w=2, tlen=N // 2 - 1)


# ---- handshake: the GEMM epilogues' partial sums on exact integer operands ----------------------------------------------------------------
def _tile_stats(C, width):
    """exact (sum, sum of squares) of every `width`-column tile of the integer matrix C (float64) -> [M, tiles, 2]"""
    M, N = C.shape
    pad = (-N) % width
    t = torch.nn.functional.pad(C, (0, pad)).view(M, -1, width)
    return torch.stack([t.sum(-1), (t * t).sum(-1)], -1)


@pytest.mark.parametrize("B,tokens,H,Hkv,K,grid_w", [(2, 64, 8, 8, 384, 8), (2, 256, 32, 32, 1536, 16)])
def test_rowstat_slots_are_the_exact_tile_sums(B, tokens, H, Hkv, K, grid_w):
    """lt_op_qkv_attention_small on integer operands: every (sum, sum of squares) slot equals the integer sums of its 128-column tile"""
    hd = 48
    d, dkv = H * hd, Hkv * hd
    M, N = B * tokens, d + 2 * dkv
    A, W, _ = XO.operands(M, N, K, torch.Generator(device="cuda").manual_seed(M + K))
    want = XO.expected(A, W).double()
    ones, zeros = bf(torch.ones(d)), bf(torch.zeros(d))
    table, _ = E.quarter_turn_table(2, 40, hd, 1, "cuda")
    slots = (N + 127) // 128
    C = XO.Guarded(M, N)
    ws = torch.full((M, slots, 2), float("nan"), device="cuda", dtype=torch.float32)
    out = XO.Guarded(M, d)
    ok(lib().lt_op_qkv_attention_small(P(A), P(W), P(C.out), M, K, H, Hkv, tokens, hd, P(ones), P(zeros), P(ones), P(zeros), P(table), 40, grid_w, 1.0,
                                       P(ws), P(out.out), stream()), "qkv_attention_small")
    torch.cuda.synchronize()
    C.assert_intact("C")
    out.assert_intact("out")
    XO.assert_words_equal(C.out, want.to(torch.bfloat16), "small-M QKV GEMM")
    exact = _tile_stats(want, 128)
    assert float(exact[..., 1].max()) < XO.FP32_EXACT
    assert torch.equal(ws.double(), exact), f"{int((ws.double() != exact).sum())} of {exact.numel()} rowstat words differ from the integer sums"


@pytest.mark.parametrize("B,tokens,H,Hkv,grid_w", [(2, 4096, 32, 32, 64)])
def test_qstat_slots_are_the_exact_half_tile_sums(B, tokens, H, Hkv, grid_w):
    """lt_op_qkv_qstat on integer operands: the workspace holds [M][slots] (sum, sum of squares), one slot per half column tile of the Q
    columns (tiles 256 or 288 wide); every word equals the integer sums"""
    hd = 72
    d, dkv = H * hd, Hkv * hd
    M, N, K, split = B * tokens, d + 2 * dkv, d, d + dkv
    assert lib().lt_op_gemm_qkv_fusable(M, N, K, split, tokens, hd) == 1
    A, W, _ = XO.operands(M, N, K, torch.Generator(device="cuda").manual_seed(M + K))
    want = XO.expected(A, W).double()
    kw, kb = bf(torch.ones(dkv)), bf(torch.zeros(dkv))
    table, _ = E.quarter_turn_table(2, 70, hd, 1, "cuda")
    gc, gv = XO.Guarded(M, N), XO.Guarded(B * Hkv * hd, tokens)
    k1 = torch.empty(B, Hkv, tokens, hd, device="cuda", dtype=torch.bfloat16)
    ws = torch.full((M * 32, 2), float("nan"), device="cuda", dtype=torch.float32)
    qmr = torch.empty(M, 2, device="cuda", dtype=torch.float32)
    ok(lib().lt_op_qkv_qstat(P(A), P(W), P(gc.out), P(gv.out), M, N, K, split, tokens, hd, d, P(kw), P(kb), P(table[1]), grid_w, 1.0,
                             P(k1), P(ws), P(qmr), stream()), "qkv_qstat")
    torch.cuda.synchronize()
    gc.assert_intact("C")
    gv.assert_intact("vt")
    written = int((~torch.isnan(ws[:, 0])).sum())
    assert written % M == 0 and bool((~torch.isnan(ws[:written])).all()), "the written slots are not one dense [M][slots] block"
    slots = written // M
    assert slots > 0 and (2 * d) % slots == 0 and 2 * d // slots in (256, 288), (slots, d)
    exact = _tile_stats(want[:, :d], d // slots)
    assert float(exact[..., 1].max()) < XO.FP32_EXACT
    got = ws[:written].view(M, slots, 2).double()
    assert torch.equal(got, exact), f"{int((got != exact).sum())} of {exact.numel()} qstat words differ from the integer sums"
