"""CPU: tests/exact_rows.py checked on itself.  (1) The fp32 emulations of every row-kernel chain - the statistic summed in the kernel's own
order, serially and pairwise - pass the word-exact comparator with zero wrong words, and the statistic's measured fp32 error stays below the
bound derived from the operation counts.  (2) Planted local faults are each caught and located - among them one the rel-L2 gates of
tests/test_gpu_ops.py let through."""
import pytest
import torch

import exact_rows as R
from exact_operands import PreconditionError

ORDERS = ["kernel", "serial", "pairwise"]
EPS = 1e-5


def _mod_inputs(B, N, d, seed, ld_extra=16):
    x = R.draw_rows(B * N, d, seed)
    w = R.draw_vec(d, seed + 1, 1.0)
    ld = 3 * d + ld_extra
    mod = R.draw_mod(B, ld, seed + 2)
    return x, w, mod[:, 8:8 + d], mod[:, 8 + d:8 + 2 * d]


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---- (1) the emulations pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 520, 576, 1536, 2304, 3072, 4096])
def test_measured_fp32_statistic_error_is_below_the_derived_bound(d):
    """three summation orders of sum(x^2), of the mean and of the centred sum of squares against float64: the worst relative error of
    rinv / rstd and the worst mean error over mean|x| stay below the derived (unmargined) bounds"""
    x = R.draw_rows(33, d, d, mean_rows=True)
    x64 = x.double()
    want = R.rms_rinv(x64, EPS)
    mean64, rstd64, mabs = R.ln_stats(x64, EPS)
    for order in ORDERS:
        got = R.emu_rinv(x, EPS, order).double()
        assert float(((got - want) / want).abs().max()) < R.RMS_DERIVED, (order, d)
        mean = R.emu_sum(x, order) / float(d)
        assert float(((mean.double() - mean64).abs() / mabs).max()) < R.ln_derived(d)[0], (order, d)
        dl = x.float() - mean
        rstd = torch.rsqrt(R.emu_sum(dl * dl, order) / float(d) + torch.tensor(EPS))
        assert float(((rstd.double() - rstd64) / rstd64).abs().max()) < R.ln_derived(d)[1], (order, d)
    assert R.DELTA_RMS == 4 * R.RMS_DERIVED == 2.0 ** -18 and R.ln_bounds(4096)[0] == 160 * R.U


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("d", [8, 520, 2304, 4096])
@pytest.mark.parametrize("use", [(1, 1, 1, 0, 0), (1, 1, 0, 1, 0), (0, 1, 1, 0, 0), (1, 0, 0, 0, 0), (0, 0, 0, 0, 0), (1, 1, 1, 0, 1)])
def test_rmsnorm_mod_emulation_is_word_exact(d, use, order):
    has_w, has_scale, has_shift, scale_pre, apex = use
    B, N = 3, 5
    x, w, scale, shift = _mod_inputs(B, N, d, d + 7)
    w, scale, shift = (w if has_w else None), (scale if has_scale else None), (shift if has_shift else None)
    got = R.emu_rmsnorm_mod(x, w, scale, shift, B, N, EPS, scale_pre, apex, order)
    ch = R.ref_rmsnorm_mod(x, w, scale, shift, B, N, EPS, scale_pre, apex)
    assert R.assert_row_words(got, ch, f"emu rmsnorm_mod {d} {use} {order}", N=N) <= R.MAX_AMBIGUOUS


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("d", [576, 1536])
@pytest.mark.parametrize("post_mode,next_mode,apex", [(1, 1, 0), (1, 2, 0), (0, 1, 0), (0, 2, 0), (1, 0, 0), (1, 1, 1)])
def test_gated_residual_norm_emulation_is_word_exact(d, post_mode, next_mode, apex, order):
    B, N = 3, 5
    x, y = R.draw_rows(B * N, d, d, std=1.0, mean_rows=True), R.draw_rows(B * N, d, d + 1, std=2.0)
    pw, nw = R.draw_vec(d, 3, 1.0), R.draw_vec(d, 4, 1.0)
    mod = R.draw_mod(B, 4 * d, 5)
    gate, ns, nsh = mod[:, :d], (1.0 + mod[:, d:2 * d].float()).to(torch.bfloat16), mod[:, 2 * d:3 * d]
    xn, h = R.emu_gated(x, y, pw, gate, nw if next_mode == 1 else None, ns, nsh, B, N, EPS, 1e-6, post_mode, next_mode, 1, apex, order)
    what = f"emu gated {d} {post_mode} {next_mode} {apex} {order}"
    R.assert_row_words(xn, R.ref_gated_x(x, y, pw, gate, B, N, EPS, post_mode, apex), what + " x", N=N)
    if next_mode:
        R.assert_row_words(h, R.ref_gated_h(xn, nw if next_mode == 1 else None, ns, nsh, B, N, EPS, 1e-6, next_mode, 1, apex), what + " h", N=N)


@pytest.mark.parametrize("slots", [12, 18])
def test_streaming_emulation_with_given_partials_is_word_exact(slots):
    B, N, d = 1, 7, 1536
    x, y = R.draw_rows(B * N, d, 1, std=1.0), R.draw_rows(B * N, d, 2, std=2.0)
    sq = y.float() ** 2
    bounds = [d * s // slots // 8 * 8 for s in range(slots)] + [d]
    ystat = torch.stack([sq[:, bounds[s]:bounds[s + 1]].sum(-1) for s in range(slots)], -1)
    pw, nw, mod = R.draw_vec(d, 3, 1.0), R.draw_vec(d, 4, 1.0), R.draw_mod(B, 2 * d, 5)
    xn, h = R.emu_gated(x, y, pw, mod[:, :d], nw, mod[:, d:], None, B, N, EPS, 1e-6, 1, 1, 1, 0, "kernel", ystat)
    R.assert_row_words(xn, R.ref_gated_x(x, y, pw, mod[:, :d], B, N, EPS, 1, 0, ystat), "emu ystat x", N=N)
    R.assert_row_words(h, R.ref_gated_h(xn, nw, mod[:, d:], None, B, N, EPS, 1e-6, 1), "emu ystat h", N=N)


def _moe_inputs(rows, d, seed):
    g = torch.Generator().manual_seed(seed)
    ys = R.draw_rows(2 * rows + 6, d, seed, std=2.0)
    pos = torch.randperm(2 * rows + 6, generator=g)[:2 * rows].view(rows, 2).int()      # a permutation with gaps (padding rows)
    wa = torch.rand(rows, 1, generator=g) * 0.6 + 0.2
    return ys, pos, torch.cat([wa, 1 - wa], 1).to(torch.bfloat16)


def test_moe_combine_emulation_is_word_exact():
    rows, d = 15, 1536
    ys, pos, wts = _moe_inputs(rows, d, 3)
    y = R.emu_moe_combine(ys, pos, wts)
    assert torch.equal(y.double(), R.moe_combine(ys, pos, wts))


def _qk_inputs(B, N, heads, hd, seed, mean_rows=True):
    width = heads * hd
    src = R.draw_rows(B * N, width + 64, seed, std=1.0, mean_rows=mean_rows)
    return src, R.draw_vec(width, seed + 1, 1.0), R.draw_vec(width, seed + 2, 0.0)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("heads,hd,qk_norm,rope_mode,osc,packed", [(2, 72, 1, 1, 1.0, 0), (8, 72, 1, 1, 0.1875, 1), (32, 128, 1, 2, 1.0, 0), (32, 48, 0, 1, 1.0, 0),
                                                                 (16, 96, 1, 0, 0.1875, 0), (2, 72, 0, 0, 1.0, 0)])
def test_qk_norm_rope_emulation_is_word_exact(heads, hd, qk_norm, rope_mode, osc, packed, order):
    B, N, gw = 2, 60, 10
    src, w, b = _qk_inputs(B, N, heads, hd, heads + hd)
    table = R.rope_table(64, hd // 4 if rope_mode == 1 else hd // 2)
    ntok, gwb = (torch.tensor([60, 35]), torch.tensor([10, 7])) if packed else (None, None)
    args = (src, 64, w if qk_norm else None, b if qk_norm else None, EPS, B, N, heads, hd, rope_mode, table, 1, gw, osc, ntok, gwb)
    got = R.emu_qk_norm_rope(*args, order=order)
    R.assert_row_words(got, R.ref_qk_norm_rope(*args), f"emu qk {heads}x{hd} {order}", N=N, hd=hd)


# ---- (2) planted faults -----------------------------------------------------------------------------------------------------------------
def _caught(got, ch, **kw):
    with pytest.raises(AssertionError) as e:
        R.assert_row_words(got, ch, "planted", **kw)
    return str(e.value), R.wrong_mask(got, ch)


def test_one_element_missing_from_a_sum_of_squares_passes_the_old_gate_and_is_caught():
    B, N, d = 2, 33, 2304
    x, w, scale, _ = _mod_inputs(B, N, d, 1)
    row = 7
    col = int(x[row].float().abs().argmax())
    got = R.emu_rmsnorm_mod(x, w, scale, None, B, N, EPS, drop=(row, col))
    ch = R.ref_rmsnorm_mod(x, w, scale, None, B, N, EPS)
    assert _rel_l2(got, ch.want) < 2e-3                                   # the gate of test_gpu_ops.py::test_rmsnorm_mod
    msg, bad = _caught(got, ch, N=N)
    assert bad[row].sum() > 20 and not bad[torch.arange(B * N) != row].any() and f"row {{{row}:" in msg, msg
    # the same fault in every row: still under the old gate
    rows = torch.arange(B * N)
    got = R.emu_rmsnorm_mod(x, w, scale, None, B, N, EPS, drop=(rows, (7 * rows + 11) % d))
    assert _rel_l2(got, ch.want) < 2e-3 and R.wrong_mask(got, ch).double().mean() > 0.005


def test_boundary_row_modulated_with_the_next_samples_scale_is_located():
    B, N, d = 3, 5, 576
    x, w, scale, shift = _mod_inputs(B, N, d, 2)
    got = R.emu_rmsnorm_mod(x, w, scale, shift, B, N, EPS, fault="boundary_scale")
    msg, bad = _caught(got, R.ref_rmsnorm_mod(x, w, scale, shift, B, N, EPS), N=N)
    assert bad[N - 1].sum() > d // 4 and not bad[torch.arange(B * N) != N - 1].any() and f"row {{{N - 1}:" in msg and "sample {0:" in msg, msg


def test_apex_order_in_place_of_the_vanilla_one_is_caught():
    B, N, d = 3, 5, 576
    x, w, scale, _ = _mod_inputs(B, N, d, 3)
    got = R.emu_rmsnorm_mod(x, w, scale, None, B, N, EPS, apex=1)
    _, bad = _caught(got, R.ref_rmsnorm_mod(x, w, scale, None, B, N, EPS, apex=0), N=N)
    assert bad.any(1).all()                                               # every row has wrong words: not a local fault
    R.assert_row_words(got, R.ref_rmsnorm_mod(x, w, scale, None, B, N, EPS, apex=1), "apex against its own chain")


def test_missing_rounding_of_one_plus_scale_is_caught():
    B, N, d = 3, 5, 576
    x, w, scale, _ = _mod_inputs(B, N, d, 4)
    got = R.emu_rmsnorm_mod(x, w, scale, None, B, N, EPS, fault="no_round_one_plus")
    _caught(got, R.ref_rmsnorm_mod(x, w, scale, None, B, N, EPS), N=N)


def test_row_and_column_position_swapped_for_one_complex_slot_is_located():
    B, N, heads, hd = 2, 60, 8, 72
    src, w, b = _qk_inputs(B, N, heads, hd, 5)
    table = R.rope_table(64, hd // 4)
    args = (src, 64, w, b, EPS, B, N, heads, hd, 1, table, 1, 10, 1.0)
    got = R.emu_qk_norm_rope(*args, fault="swap_row_col")
    msg, bad = _caught(got, R.ref_qk_norm_rope(*args), N=N, hd=hd)
    cols = bad.any(0).nonzero().flatten()
    assert set((cols % hd).tolist()) == {2, 3} and set((cols // hd).tolist()) == set(range(heads)), msg


def test_padded_token_rotating_with_its_own_index_is_located():
    B, N, heads, hd = 2, 60, 2, 72
    src, w, b = _qk_inputs(B, N, heads, hd, 6)
    table = R.rope_table(64, hd // 4)
    ntok, gwb = torch.tensor([60, 35]), torch.tensor([10, 7])
    args = (src, 64, w, b, EPS, B, N, heads, hd, 1, table, 1, 10, 1.0, ntok, gwb)
    got = R.emu_qk_norm_rope(*args, fault="pad_own_index")
    msg, bad = _caught(got, R.ref_qk_norm_rope(*args), N=N, hd=hd)
    rows = bad.any(1).nonzero().flatten().tolist()
    assert rows == list(range(N + 35, 2 * N)) and "sample {1:" in msg, (rows, msg)


def test_pair_layout_piece_at_the_other_rows_address_is_located():
    B, N, d = 2, 7, 576
    x, w, scale, _ = _mod_inputs(B, N, d, 7)
    out = R.emu_rmsnorm_mod(x, w, scale, None, B, N, EPS)
    pair = out.view(B * N // 2, 2, d // 32, 32).permute(0, 2, 1, 3).contiguous()      # [pair, piece, row & 1, 32]
    assert torch.equal(R.from_pair(pair.view(-1), B * N, d), out)
    pair[1, 2] = pair[1, 2].flip(0)                                                   # piece 2 of rows 2 / 3 at the other row's address
    msg, bad = _caught(R.from_pair(pair.view(-1), B * N, d), R.ref_rmsnorm_mod(x, w, scale, None, B, N, EPS), N=N)
    idx = bad.nonzero()
    assert set(idx[:, 0].tolist()) == {2, 3} and int(idx[:, 1].min()) >= 64 and int(idx[:, 1].max()) < 96, msg


def test_moe_weights_paired_with_the_wrong_expert_row_are_located():
    rows, d = 15, 1536
    ys, pos, wts = _moe_inputs(rows, d, 8)
    x = R.draw_rows(rows, d, 9, std=1.0)
    pw, mod = R.draw_vec(d, 3, 1.0), R.draw_mod(3, d, 5)
    y_bad = R.emu_moe_combine(ys, pos, wts, fault="moe_wrong_row")
    xn, _ = R.emu_gated(x, y_bad, pw, mod, None, None, None, 3, 5, EPS, 1e-6, 1, 0)
    y = R.moe_combine(ys, pos, wts).to(torch.bfloat16)
    msg, bad = _caught(xn, R.ref_gated_x(x, y, pw, mod, 3, 5, EPS), N=5)
    assert bad[2].sum() > d // 4 and not bad[torch.arange(rows) != 2].any() and "row {2:" in msg, msg


def test_unwritten_chunk_is_counted_and_located():
    B, N, d = 3, 5, 520
    x, w, scale, _ = _mod_inputs(B, N, d, 10)
    got = R.emu_rmsnorm_mod(x, w, scale, None, B, N, EPS)
    got[3, 512:520] = float("nan")                                        # the one live lane of the second chunk round
    msg, _ = _caught(got, R.ref_rmsnorm_mod(x, w, scale, None, B, N, EPS), N=N)
    assert "8 of" in msg and "(8 unwritten" in msg and "chunk {64: 8}" in msg and "lane {0: 8}" in msg and "chunk / 64 {1: 8}" in msg, msg


def test_stray_store_into_a_guard_is_reported():
    g = R.GuardedBuf(15 * 520, device="cpu")
    g.assert_intact("clean")
    g.buf[g.zone + g.n + 5] = 1.0
    with pytest.raises(AssertionError, match=r"0 words before it, 1 behind it \(first at \+5 words\)"):
        g.assert_intact("stray")
    g2, view = R.guarded_copy(torch.ones(3, 8, dtype=torch.bfloat16), device="cpu")
    g2.buf[g2.zone - 1] = 0.0
    with pytest.raises(AssertionError, match="1 words before it"):
        g2.assert_intact("stray")


def test_too_many_ambiguous_words_is_a_precondition_error_not_a_looser_comparison():
    x = R.draw_rows(4, 64, 1)
    ch = R.Chain(x.shape).round(lambda _: x.double(), rel=2.0 ** -9)      # every word within the bound of a midpoint
    ch.amb[:] = True
    with pytest.raises(PreconditionError):
        R.assert_row_words(x, ch, "cap")


def test_routing_check_accepts_the_float64_router_and_rejects_a_swapped_pair():
    rows, d, E = 15, 1536, 8
    h = R.draw_rows(rows, d, 11, std=1.0)
    rw = R.draw_vec(E * d, 12, 0.0, 0.05).view(E, d)
    logits = R.rn(h.double() @ rw.double().t())
    top = torch.topk(logits, 2, dim=1).indices.sort(1).values
    l0, l1 = logits.gather(1, top[:, 0:1]), logits.gather(1, top[:, 1:2])
    w0 = 1.0 / (1.0 + torch.exp(l1 - l0))
    wts = torch.cat([w0, 1.0 - w0], 1).to(torch.bfloat16)
    R.check_routing(h, rw, top.int(), wts, what="float64 router")
    with pytest.raises(AssertionError, match="routing wrong on"):
        R.check_routing(h, rw, top.int(), wts.flip(1), what="swapped")
