"""-m gpu: the ragged boundary kernels of a packed batch (csrc/packed.hip) through their lt_op_* entries.  One launch serves all samples; per
sample the result must be, word for word, what the tensor kernel's entry (lt_op_patchify / lt_op_fill_rows_bf16 / lt_op_unpatchify_cfg)
gives on that sample alone.  Destinations are poisoned with NaN: every word outside a sample's region must keep the poison, except pad rows,
which must hold pad_token.

Sizes: latents 12x20, 16x16, 6x16 (60, 64, 24 tokens: two non-square, the longest not first, one count no multiple of 64, one under half a
tile, three widths) plus 2x16, a single patch row.  Movement is checked on integer-valued words, the guidance chain on the operands the
tensor kernel's own exact test draws (exact_rows.draw_rows, as tests/test_gpu_misc_exact.py does) and against exact_misc's chain reference.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_misc as M
import exact_rows as R
from gpu_util import P, lib, ok, stream

pytestmark = pytest.mark.gpu

SIZES = [(12, 20), (16, 16), (6, 16), (2, 16)]
CH, PATCH, KPAD, GUARD = 4, 2, 32, 64
DT = {0: torch.float32, 1: torch.bfloat16}


def _hw(sizes):
    return (C.c_int32 * (2 * len(sizes)))(*[v for s in sizes for v in s])


def _ntok(s):
    return (s[0] // PATCH) * (s[1] // PATCH)


def _tab():
    return torch.zeros(5 * 64, dtype=torch.int32, device="cuda")


def _poison(n, dtype=torch.bfloat16):
    return torch.full((n,), float("nan"), dtype=dtype, device="cuda")


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _same_words(a, b):
    return np.array_equal(M.bits(a), M.bits(b))


@pytest.mark.parametrize("dup", [0, 1])
@pytest.mark.parametrize("xd", [1, 0])
@pytest.mark.parametrize("N", [64, 70])
def test_patchify_packed_equals_the_tensor_kernel_per_sample(xd, dup, N):
    sizes = SIZES * 2 if dup else SIZES
    B = len(sizes)
    gen = torch.Generator().manual_seed(11 + xd)
    xs = [torch.randint(-120, 121, (CH,) + s, generator=gen).to(DT[xd]).cuda() for s in sizes]
    flat = torch.cat([x.reshape(-1) for x in xs])
    out = _poison((B * N + 2) * KPAD).view(B * N + 2, KPAD)  # one guard row on each side
    ok(lib().lt_op_patchify_packed(P(flat), xd, P(out[1:]), _hw(sizes), P(_tab()), B, CH, PATCH, KPAD, N, dup, stream()), "patchify_packed")
    torch.cuda.synchronize()
    assert _all_nan(out[0]) and _all_nan(out[-1])
    body = out[1:-1].view(B, N, KPAD)
    for b, s in enumerate(sizes):
        src = xs[b % (B // 2)] if dup else xs[b]
        n = _ntok(s)
        solo = _poison(n * KPAD).view(n, KPAD)
        ok(lib().lt_op_patchify(P(src.contiguous()), xd, P(solo), 1, CH, s[0], s[1], PATCH, KPAD, 0, 0, stream()), "patchify")
        torch.cuda.synchronize()
        assert not torch.isnan(solo.float()).any()
        assert _same_words(body[b, :n], solo), (b, s)
        assert _all_nan(body[b, n:]), (b, s)  # rows behind the last token are not this kernel's to write
        # the movement itself, on the integer words: token (i, j), column (c, ph, pw)
        want = src.float().view(CH, s[0] // PATCH, PATCH, s[1] // PATCH, PATCH).permute(1, 3, 0, 2, 4).reshape(n, CH * PATCH * PATCH)
        assert torch.equal(body[b, :n, :CH * PATCH * PATCH].float(), want) and not body[b, :n, CH * PATCH * PATCH:].any()


@pytest.mark.parametrize("N,d", [(64, 72), (70, 576)])
def test_fill_pad_packed_writes_the_pad_rows_only(N, d):
    B = len(SIZES)
    pad = R.draw_rows(1, d, 5, std=1.0).reshape(-1).cuda()
    x = _poison((B * N + 2) * d).view(B * N + 2, d)
    ok(lib().lt_op_fill_pad_packed(P(x[1:]), P(pad), _hw(SIZES), P(_tab()), B, PATCH, N, d, stream()), "fill_pad_packed")
    torch.cuda.synchronize()
    assert _all_nan(x[0]) and _all_nan(x[-1])
    body = x[1:-1].view(B, N, d)
    for b, s in enumerate(SIZES):
        n = _ntok(s)
        assert _all_nan(body[b, :n]), (b, s)
        solo = _poison((N - n) * d).view(N - n, d)
        if N > n:
            ok(lib().lt_op_fill_rows_bf16(P(solo), P(pad), N - n, d, stream()), "fill_rows_bf16")
            torch.cuda.synchronize()
        assert _same_words(body[b, n:], solo) and _same_words(body[b, n:], pad.expand(N - n, d)), (b, s)


# (out dtype, out_ch, extra ld, use_cfg, cfg_scale, cfg_channels)
UNPATCH = [(1, 8, 0, 1, 4.0, 3), (0, 8, 8, 1, 4.3, 3), (1, 8, 8, 1, 4.3, 4), (1, 8, 0, 0, 1.0, 3), (0, 4, 0, 0, 1.0, 4)]


@pytest.mark.parametrize("c", UNPATCH, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("N", [64, 70])
def test_unpatchify_packed_equals_the_tensor_kernel_per_sample(c, N):
    od, och, extra, use_cfg, scale, cfgc = c
    sizes = SIZES * 2 if use_cfg else SIZES
    B, half = len(sizes), len(sizes) // 2
    ld = PATCH * PATCH * och + extra
    rows = R.draw_rows(B * N, ld, 31 + sum(map(int, c[:4])) + N, std=1.0)
    rg = rows.cuda()
    total = sum(CH * s[0] * s[1] for s in sizes)
    buf = _poison(total + 2 * GUARD, DT[od])
    ok(lib().lt_op_unpatchify_packed(P(rg), ld, P(buf[GUARD:]), od, _hw(sizes), P(_tab()), B, CH, och, PATCH, N, use_cfg, scale, cfgc, stream()),
       "unpatchify_packed")
    torch.cuda.synchronize()
    assert _all_nan(buf[:GUARD]) and _all_nan(buf[GUARD + total:])
    assert torch.equal(rg.cpu(), rows)
    off = GUARD
    for b, s in enumerate(sizes):
        n, sz = _ntok(s), CH * s[0] * s[1]
        got = buf[off:off + sz].view(CH, s[0], s[1])
        off += sz
        if use_cfg:  # the pair (cond row, uncond row) of this sample as a batch of 2
            pair = torch.cat([rows[(b % half) * N:(b % half) * N + n], rows[(b % half + half) * N:(b % half + half) * N + n]]).contiguous()
            nb, pick = 2, (0 if b < half else 1)
        else:
            pair, nb, pick = rows[b * N:b * N + n].contiguous(), 1, 0
        solo = _poison(nb * sz, DT[od]).view(nb, CH, s[0], s[1])
        ok(lib().lt_op_unpatchify_cfg(P(pair.cuda()), ld, P(solo), od, nb, CH, och, s[0], s[1], PATCH, use_cfg, scale, cfgc, 0, stream()), "unpatchify_cfg")
        torch.cuda.synchronize()
        assert not torch.isnan(solo.float()).any()
        assert _same_words(got, solo[pick]), (b, s)
        # ... and the chain reference of the tensor kernel's own exact test
        ch = M.ref_unpatchify_cfg(pair, nb, CH, och, s[0], s[1], PATCH, use_cfg, scale, cfgc, 0)
        both = solo.clone()
        both[pick] = got
        (M.assert_words if od else M.assert_f32_holds_bf16)(both.reshape(nb * CH, -1), ch, f"unpatchify_packed {c} sample {b}")


def test_packed_op_entries_refuse_bad_size_lists():
    tab, buf = _tab(), _poison(64 * KPAD * 4)
    x = torch.zeros(4 * 16 * 16, dtype=torch.bfloat16, device="cuda")
    L = lib()
    assert L.lt_op_patchify_packed(P(x), 1, P(buf), _hw([(15, 16)]), P(tab), 1, CH, PATCH, KPAD, 64, 0, stream()) != 0
    assert b"multiple of the patch" in L.lt_last_error()
    assert L.lt_op_patchify_packed(P(x), 1, P(buf), _hw([(16, 16)]), P(tab), 1, CH, PATCH, KPAD, 63, 0, stream()) != 0
    assert b"longest sample" in L.lt_last_error()
    assert L.lt_op_patchify_packed(P(x), 1, P(buf), _hw([(16, 16)] * 65), P(tab), 65, CH, PATCH, KPAD, 64, 0, stream()) != 0
    assert L.lt_op_unpatchify_packed(P(buf), 32, P(x), 1, _hw([(16, 16), (8, 16)]), P(tab), 2, CH, 8, PATCH, 64, 1, 4.0, 3, stream()) != 0
    assert b"halves differ" in L.lt_last_error()
    torch.cuda.synchronize()
    assert _all_nan(buf)
