"""The MoE routing plan (integer / index work): oracle/moe_plan_oracle.py against the reference's expert loop semantics (CPU), and
lt_op_moe_plan against the oracle BIT FOR BIT (GPU) - every register form of the kernel (4 / 8 / 16 / 32 entries per thread), the
generic walk beyond 16 384 rows, empty experts, everything on two experts, one row, ragged counts, ties in the time router.
lt_op_moe_plan_ex (every field of MoeArgs) reaches what lt_op_moe_plan cannot: the time router on the single-workgroup kernel (more than 64
samples, or a forced table whose rows choose differently inside a sample) in every register form and the generic walk, and the all-layers
form of the closed-form time plan (three layers, padded strides with sentinels between the slices, each layer against the single-layer
call on its own logit columns) with its refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import moe_plan_oracle as MP


def _random_sel(rows, E, seed, mode="uniform"):
    rng = np.random.default_rng(seed)
    if mode == "two":  # every row picks experts (0, 1): two full segments, the rest empty
        sel = np.tile(np.array([[0, 1]], dtype=np.int32), (rows, 1))
    elif mode == "skewed":  # expert E - 1 is never chosen, expert 0 almost always
        a = np.zeros(rows, dtype=np.int32)
        b = rng.integers(1, max(2, E - 1), rows).astype(np.int32)
        sel = np.stack([a, b], 1)
    else:
        a = rng.integers(0, E, rows)
        b = (a + rng.integers(1, E, rows)) % E
        sel = np.sort(np.stack([a, b], 1), axis=1).astype(np.int32)
    return sel


@pytest.mark.parametrize("rows,E,mode", [(1, 2, "uniform"), (300, 4, "uniform"), (1000, 8, "skewed"), (512, 4, "two")])
def test_plan_oracle_is_the_reference_expert_loop(rows, E, mode):
    """Next-DiT-MoE/models/models2.py:470-476: `for i, expert in enumerate(experts): rows_i, nth = torch.where(selected == i);
    results[rows_i] += w[rows_i, nth] * expert(x[rows_i])`.  Running the experts over the oracle's sorted layout (gather through
    src, one 'expert' per tile through tile_expert, scatter-add back through pos in ascending expert order) must give the same
    tensor as that loop - with an expert function that depends on the expert id and on the row."""
    sel = _random_sel(rows, E, 3 + rows, mode)
    max_tiles = (2 * rows + E * 255 + 255) // 256
    pos, src, te = MP.plan(sel, E, max_tiles)
    # structure: pos is a bijection onto the non-padding positions, segments are tile-aligned, in expert order, stable
    flat = pos.reshape(-1)
    assert len(set(flat.tolist())) == 2 * rows and (src[flat] == np.repeat(np.arange(rows), 2)).all()
    assert (src >= 0).sum() == 2 * rows
    for e in range(E):
        idx = np.nonzero(sel.reshape(-1) == e)[0]
        if idx.size:
            q = flat[idx]
            assert q[0] % 256 == 0 and (np.diff(q) == 1).all() and (te[q // 256] == e).all()
    x = torch.randn(rows, 8, generator=torch.Generator().manual_seed(rows))
    w = torch.rand(rows, 2, generator=torch.Generator().manual_seed(rows + 1))
    expert = lambda e, v: v * (e + 1) + e
    want = torch.zeros_like(x)
    tsel = torch.from_numpy(sel)
    for e in range(E):  # the reference loop
        r, nth = torch.where(tsel == e)
        if r.numel():
            want[r] += w[r, nth, None] * expert(e, x[r])
    xs = torch.zeros(max_tiles * 256, 8)
    valid = src >= 0
    xs[valid] = x[src[valid]]
    ys = torch.zeros_like(xs)
    for t_, e in enumerate(te):
        if e >= 0:
            ys[256 * t_: 256 * t_ + 256] = expert(int(e), xs[256 * t_: 256 * t_ + 256])
    got = w[:, 0, None] * ys[pos[:, 0]] + w[:, 1, None] * ys[pos[:, 1]]  # ascending expert id = the loop's accumulation order
    assert torch.allclose(got, want, rtol=0, atol=1e-5)


def test_time_router_oracle_ties_and_order():
    logits = np.array([[1.0, 1.0, 0.5, 1.0], [0.25, -1.0, 3.0, 3.0], [-2.0, -2.0, -2.0, -2.0]], dtype=np.float32)
    sel, wts = MP.route_time(logits, 3)
    assert sel.shape == (9, 2) and (sel[0] == [0, 1]).all() and (sel[3] == [2, 3]).all() and (sel[6] == [0, 1]).all()
    assert np.allclose(wts[0], [0.5, 0.5]) and np.allclose(wts.sum(1), 1.0, atol=1e-2)
    # rows without a tie among the candidates: torch.topk (what the reference calls, models2.py:464) agrees; on exact ties torch's pick is
    # implementation-defined (this CPU build returns experts (1, 3) for row 0, CUDA's radix select something else again) - the engine
    # and this oracle take the lowest indices, stated in both headers
    clear = np.array([[0.3, 2.0, -1.0, 0.9], [5.0, 4.0, 3.0, 2.0]], dtype=np.float32)
    s2, _ = MP.route_time(clear, 1)
    assert (np.sort(torch.topk(torch.from_numpy(clear), 2).indices.numpy(), 1) == s2).all()


# ---- GPU: the kernel against the oracle, bit for bit --------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _run_plan(sel, E, logits=None, rows_per_sample=0):
    from gpu_util import P, lib, ok, stream
    rows = sel.shape[0] if sel is not None else logits.shape[0] * rows_per_sample
    max_tiles = (2 * rows + E * 255 + 255) // 256
    dsel = torch.full((2 * rows + 4,), -7, dtype=torch.int32, device="cuda")
    if sel is not None:
        dsel[: 2 * rows] = torch.from_numpy(sel.reshape(-1)).cuda()
    pos = torch.full((2 * rows + 4,), -9, dtype=torch.int32, device="cuda")
    src = torch.full((max_tiles * 256,), -5, dtype=torch.int32, device="cuda")
    te = torch.full((max_tiles,), -5, dtype=torch.int32, device="cuda")
    wts = torch.zeros(2 * rows + 4, dtype=torch.bfloat16, device="cuda")
    dl = None if logits is None else torch.from_numpy(logits).to("cuda", torch.bfloat16).contiguous()
    ok(lib().lt_op_moe_plan(P(dsel), P(dl), P(wts), rows, rows_per_sample, E, P(pos), P(src), P(te), max_tiles, stream()), "moe_plan")
    torch.cuda.synchronize()
    assert (pos[2 * rows:] == -9).all(), "pos written past the last entry"
    return (dsel[: 2 * rows].view(rows, 2).cpu().numpy(), wts[: 2 * rows].float().view(rows, 2).cpu().numpy(), pos[: 2 * rows].view(rows, 2).cpu().numpy(),
            src.cpu().numpy(), te.cpu().numpy(), max_tiles)


@gpu
@pytest.mark.parametrize("rows,E,mode", [(1, 2, "uniform"), (7, 4, "uniform"), (512, 4, "uniform"), (2047, 8, "skewed"), (2048, 4, "two"), (4096, 4, "uniform"),
                                         (8192, 4, "uniform"), (8192, 8, "two"), (16384, 4, "uniform"), (16385, 4, "uniform"), (20001, 8, "skewed"), (40000, 4, "uniform")])
def test_plan_kernel_equals_oracle_bit_for_bit(rows, E, mode):
    sel = _random_sel(rows, E, 11 + rows + E, mode)
    sel_back, _, pos, src, te, max_tiles = _run_plan(sel, E)
    want_pos, want_src, want_te = MP.plan(sel, E, max_tiles)
    assert np.array_equal(sel_back, sel)  # untouched on the space path
    assert np.array_equal(te, want_te)
    assert np.array_equal(pos, want_pos)
    assert np.array_equal(src, want_src)


@gpu
@pytest.mark.parametrize("B,rps,E", [(2, 256, 4), (2, 4096, 4), (3, 1000, 8), (8, 4096, 4), (2, 9000, 8)])
def test_plan_kernel_time_branch_routes_like_the_oracle(B, rps, E):
    rng = np.random.default_rng(B * rps + E)
    logits = torch.from_numpy(rng.normal(size=(B, E)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    logits[0, 1] = logits[0, 0] = max(logits[0].max(), 1.0)  # a tie for the first maximum: lowest index wins, the other is second
    sel, wts, pos, src, te, max_tiles = _run_plan(None, E, logits=logits, rows_per_sample=rps)
    want_sel, want_wts = MP.route_time(logits, rps)
    assert np.array_equal(sel, want_sel)
    assert np.abs(wts - want_wts).max() <= 2.0 ** -8  # bf16 weights; the kernel's exp is the hardware's v_exp_f32: <= one bf16 ulp
    want_pos, want_src, want_te = MP.plan(want_sel, E, max_tiles)
    assert np.array_equal(pos, want_pos) and np.array_equal(src, want_src) and np.array_equal(te, want_te)


# ---- lt_op_moe_plan_ex: the time router on the single-workgroup kernel, the forced table, the all-layers form ------------------------
def _logits(B, cols, seed):
    """bf16-valued logits with an exact tie for sample 0's maximum (lowest index wins)"""
    rng = np.random.default_rng(seed)
    lg = torch.from_numpy(rng.normal(size=(B, cols)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    lg[0, 1] = lg[0, 0] = max(float(lg[0].max()), 1.0)
    return lg


def _run_plan_ex(logits, rps, E, forced=None, sample_ld=0, col0=0, layers=1, stride_pad=(0, 0, 0)):
    """lt_op_moe_plan_ex on buffers whose every word outside a layer's slice holds a sentinel.  -> per layer (sel, wts, pos, src, te), max_tiles"""
    from gpu_util import P, lib, ok, stream
    B = logits.shape[0]
    rows = B * rps
    max_tiles = (2 * rows + E * 255 + 255) // 256          # moe_ffn's bound for the call's rows (csrc/engine.hip, kernels.h MoeArgs::max_tiles)
    sr, ss, st = 2 * rows + 4 + stride_pad[0], max_tiles * 256 + stride_pad[1], max_tiles + stride_pad[2]
    dsel = torch.full((layers * sr,), -7, dtype=torch.int32, device="cuda")
    pos = torch.full((layers * sr,), -9, dtype=torch.int32, device="cuda")
    wts = torch.full((layers * sr,), -3.0, dtype=torch.bfloat16, device="cuda")
    src = torch.full((layers * ss,), -5, dtype=torch.int32, device="cuda")
    te = torch.full((layers * st,), -5, dtype=torch.int32, device="cuda")
    dl = torch.from_numpy(logits).to("cuda", torch.bfloat16).contiguous()
    df = None if forced is None else torch.from_numpy(np.ascontiguousarray(forced, dtype=np.int32)).cuda()
    lp = C.c_void_p(dl.data_ptr() + 2 * col0)
    ok(lib().lt_op_moe_plan_ex(P(dsel), lp, sample_ld, P(df), P(wts), rows, rps, E, P(pos), P(src), P(te), max_tiles, layers, sr, ss, st, stream()),
       "moe_plan_ex")
    torch.cuda.synchronize()
    out = []
    for l in range(layers):
        a, b, c = dsel[l * sr:(l + 1) * sr], pos[l * sr:(l + 1) * sr], wts[l * sr:(l + 1) * sr]
        assert (a[2 * rows:] == -7).all() and (b[2 * rows:] == -9).all() and (c[2 * rows:] == -3.0).all(), f"layer {l}: a word behind the rows was written"
        s, t_ = src[l * ss:(l + 1) * ss], te[l * st:(l + 1) * st]
        assert (s[max_tiles * 256:] == -5).all() and (t_[max_tiles:] == -5).all(), f"layer {l}: a word behind the sorted positions / tiles was written"
        out.append((a[:2 * rows].view(rows, 2).cpu().numpy(), c[:2 * rows].float().view(rows, 2).cpu().numpy(), b[:2 * rows].view(rows, 2).cpu().numpy(),
                    s[:max_tiles * 256].cpu().numpy(), t_[:max_tiles].cpu().numpy()))
    return out, max_tiles


def _assert_plan(got, want_sel, want_wts, E, max_tiles, what):
    sel, wts, pos, src, te = got
    assert np.array_equal(sel, want_sel), what
    assert np.abs(wts - want_wts).max() <= 2.0 ** -8, what     # (the one bf16 ulp derived above: v_exp_f32 against numpy's exp)
    want_pos, want_src, want_te = MP.plan(want_sel, E, max_tiles)
    assert np.array_equal(pos, want_pos) and np.array_equal(src, want_src) and np.array_equal(te, want_te), what


@gpu
@pytest.mark.parametrize("B,rps,E,per", [(66, 4, 4, 4), (65, 40, 4, 8), (80, 64, 8, 16), (70, 200, 8, 32), (65, 300, 8, 0)])
def test_time_router_on_the_single_workgroup_kernel(B, rps, E, per):
    """more than 64 samples: launch_moe_plan cannot use the closed-form kernel, so moe_plan_kernel<PER> routes - the 8-byte sel stores and the
    packed weight store of the register forms, the entry-by-entry walk with its barrier of PER == 0"""
    n = 2 * B * rps
    assert B > 64 and {4: n <= 4096, 8: 4096 < n <= 8192, 16: 8192 < n <= 16384, 32: 16384 < n <= 32768, 0: n > 32768}[per]     # launch_moe_plan's dispatch
    logits = _logits(B, E, B * rps + E)
    (got,), max_tiles = _run_plan_ex(logits, rps, E)
    want_sel, want_wts = MP.route_time(logits, rps)
    _assert_plan(got, want_sel, want_wts, E, max_tiles, (B, rps, E))


def _forced_table(rows, E, seed):
    """two different experts per row, rows of one sample choosing differently, a third of the rows in descending order"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, E, rows)
    b = (a + rng.integers(1, E, rows)) % E
    f = np.sort(np.stack([a, b], 1), axis=1)
    flip = rng.integers(0, 3, rows) == 0
    f[flip] = f[flip][:, ::-1]
    return f.astype(np.int32)


@gpu
@pytest.mark.parametrize("B,rps,E", [(3, 100, 8), (8, 700, 4), (2, 9000, 8)])
def test_time_router_with_a_forced_table(B, rps, E):
    """at most 8 samples, whole samples: only the forced table keeps the call off the closed-form kernel.  Neighbouring rows of one sample take
    different experts, so a routing cached per sample would show; the weights are the softmax of the sample's logits of the FORCED experts"""
    rows = B * rps
    logits = _logits(B, E, rows + E)
    forced = _forced_table(rows, E, rows)
    assert (forced[:-1] != forced[1:]).any(1).sum() > rows // 2
    (got,), max_tiles = _run_plan_ex(logits, rps, E, forced=forced)
    want_sel, want_wts = MP.route_time_forced(logits, rps, forced)
    free_sel, _ = MP.route_time(logits, rps)
    assert (want_sel != free_sel).any(1).sum() > rows // 2        # (the table is not the free choice)
    _assert_plan(got, want_sel, want_wts, E, max_tiles, (B, rps, E))


@gpu
@pytest.mark.parametrize("B,rps,E,pad_cols", [(5, 100, 4, 0), (64, 7, 8, 5), (2, 1000, 8, 3)])
def test_all_layers_time_plan(B, rps, E, pad_cols):
    """L = 3 in one launch (blockIdx.y = layer): strides larger than a layer needs with sentinels between the slices, every layer equal to the
    oracle on its own E logit columns and, word for word, to the single-layer call on those columns; the logit rows are longer than L * E and the
    extra columns hold values that would win every top-2"""
    L = 3
    ld = L * E + pad_cols
    logits = _logits(B, ld, B * rps + E)
    logits[:, L * E:] = 64.0
    logits[1 % B, E + 2] = logits[1 % B, E + 1] = 8.0          # a tie inside layer 1's columns as well
    layers, max_tiles = _run_plan_ex(logits, rps, E, sample_ld=ld, layers=L, stride_pad=(6, 256 + 3, 5))
    for l in range(L):
        cols = np.ascontiguousarray(logits[:, l * E:(l + 1) * E])
        want_sel, want_wts = MP.route_time(cols, rps)
        _assert_plan(layers[l], want_sel, want_wts, E, max_tiles, ("layer", l))
        (single,), _ = _run_plan_ex(logits, rps, E, sample_ld=ld, col0=l * E)
        for got, one, name in zip(layers[l], single, ("sel", "wts", "pos", "src", "tile_expert")):
            assert np.array_equal(got, one), ("layer", l, name)
    if B > 1:    # (the layers are different plans: the check above could not pass by reading one layer's columns three times)
        assert any(not np.array_equal(layers[0][0], layers[l][0]) for l in (1, 2))


@gpu
def test_all_layers_form_refusals():
    from gpu_util import P, lib, stream
    E, rps, L = 4, 8, 2

    def call(B, forced):
        rows = B * rps
        max_tiles = (2 * rows + E * 255 + 255) // 256
        sr = 2 * rows + 4
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
        lg = torch.zeros(B, L * E, dtype=torch.bfloat16, device="cuda")
        f = torch.tensor([[0, 1]] * rows, dtype=torch.int32, device="cuda") if forced else None
        rc = lib().lt_op_moe_plan_ex(P(i32(L * sr)), P(lg), L * E, P(f), P(torch.zeros(L * sr, dtype=torch.bfloat16, device="cuda")), rows, rps, E, P(i32(L * sr)),
                                     P(i32(L * max_tiles * 256)), P(i32(L * max_tiles)), max_tiles, L, sr, max_tiles * 256, max_tiles, stream())
        return rc, lib().lt_last_error().decode()

    for B, forced in ((4, True), (65, False)):
        rc, msg = call(B, forced)
        assert rc != 0 and "moe_plan: the all-layers form is the time router's closed-form plan" in msg, (B, forced, rc, msg)
    rc, msg = call(4, False)
    assert rc == 0, msg
    torch.cuda.synchronize()
