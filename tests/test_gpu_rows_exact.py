"""-m gpu: the row kernels of csrc/norm.hip and csrc/qkv_post.hip against the float64 rounding-chain references of tests/exact_rows.py: every
output word must equal RN_bf16 of the chain (both neighbours only where a stage's float64 value lies within its error bound of a bf16
midpoint; DELTA_RMS = 2^-18 and the LayerNorm bounds are derived in exact_rows.py), on NaN-filled outputs between 7.0 guard zones; x is
checked in place.  The gated_residual_norm cases assert the kernel they mean to run through lt_op_gated_residual_norm_describe.  Shapes are
the smallest at which each mechanism exists: 15 rows (B = 3, N = 5: a partial last block of 4 and of 8 rows, every sample boundary inside
a block), 14 rows for the pair layouts, ld_mod > d with a column offset."""
import ctypes as C

import pytest
import torch

import exact_rows as R
from gpu_util import P, lib, ok, set_option, stream

pytestmark = pytest.mark.gpu
EPS, EPS2 = 1e-5, 1e-6
OFF = 8          # column offset of the first modulation vector inside a row of `mod`


@pytest.fixture(autouse=True)
def _default_options():
    yield
    set_option("norm_specialize", 1)
    set_option("rmsnorm_apex", 0)
    set_option("grn_ystat", 1)


class Bufs:
    """device copies between guard zones; done() synchronises and checks every guard"""

    def __init__(self):
        self.guards = []

    def put(self, t):
        if t is None:
            return None
        g, view = R.guarded_copy(t.contiguous())
        self.guards.append(g)
        return view

    def out(self, *shape, dtype=torch.bfloat16, fill=float("nan")):
        n = 1
        for s in shape:
            n *= s
        g = R.GuardedBuf(n, dtype=dtype, fill=fill)
        self.guards.append(g)
        return g.out.view(*shape)

    def done(self, what):
        torch.cuda.synchronize()
        for g in self.guards:
            g.assert_intact(what)


def _report(kernel, what, share):
    print(f"ROWS kernel={kernel} case={what} ambiguous={share:.4%}")


def _mod(B, d, nvec, seed):
    """[B, ld] with nvec vectors of d columns from column OFF on; ld > nvec * d"""
    ld = nvec * d + 24
    mod = R.draw_mod(B, ld, seed)
    return mod, ld, [mod[:, OFF + i * d:OFF + (i + 1) * d] for i in range(nvec)]


def _sub(dev_mod, i, d):
    """pointer to vector i of the device copy of mod"""
    return C.c_void_p(dev_mod.data_ptr() + 2 * (OFF + i * d))


def _describe(post_mode, next_mode, d, has_nw, has_ns, has_nsh, scale_pre, ystat_slots=0, moe=0, gate_mode=0):
    buf = C.create_string_buffer(64)
    ok(lib().lt_op_gated_residual_norm_describe(post_mode, gate_mode, next_mode, d, int(has_nw), int(has_ns), int(has_nsh), scale_pre, int(ystat_slots > 0),
                                                ystat_slots, moe, buf, 64))
    return buf.value.decode()


# ---- rmsnorm_mod ---------------------------------------------------------------------------------------------------------------------------
ALL_D = [8, 520, 576, 1536, 2304, 3072, 4096]
# (w, scale, shift, scale_pre, out_pair, apex)
RMS_CASES = [(d, u) for d in ALL_D for u in [(1, 1, 1, 0, 0, 0), (1, 1, 0, 1, 0, 0)]]
RMS_CASES += [(d, u) for d in (520, 2304) for u in [(0, 1, 1, 0, 0, 0), (1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0), (1, 0, 1, 0, 0, 0), (1, 1, 0, 0, 0, 1), (1, 0, 0, 0, 0, 1)]]
RMS_CASES += [(d, u) for d in (576, 2304, 4096) for u in [(1, 1, 0, 1, 1, 0), (1, 1, 1, 0, 1, 0)]]


@pytest.mark.parametrize("d,use", RMS_CASES, ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rmsnorm_mod_is_word_exact(d, use):
    has_w, has_scale, has_shift, scale_pre, pair, apex = use
    B, N = (2, 7) if pair else (3, 5)
    x, w = R.draw_rows(B * N, d, d + sum(use)), R.draw_vec(d, d + 1, 1.0)
    mod, ld, (scale, shift) = _mod(B, d, 2, d + 2)
    if scale_pre:
        mod[:, OFF:OFF + d] = (1.0 + scale.float()).to(torch.bfloat16)
    w, scale, shift = (w if has_w else None), (scale if has_scale else None), (shift if has_shift else None)
    b = Bufs()
    xd, wd, md, out = b.put(x), b.put(w), b.put(mod), b.out(B * N, d)
    what = f"rmsnorm_mod d {d} w/scale/shift/scale_pre/pair/apex {use}"
    set_option("rmsnorm_apex", apex)
    ok(lib().lt_op_rmsnorm_mod_ex(P(xd), P(wd), _sub(md, 0, d) if has_scale else None, _sub(md, 1, d) if has_shift else None, ld, P(out), B, N, d, EPS,
                                  scale_pre, pair, stream()), what)
    b.done(what)
    got = R.from_pair(out.cpu(), B * N, d) if pair else out
    share = R.assert_row_words(got, R.ref_rmsnorm_mod(x, w, scale, shift, B, N, EPS, scale_pre, apex), what, N=N)
    assert torch.equal(xd.cpu(), x)
    _report("rmsnorm_mod_kernel<%d>" % R.maxch(d), what, share)


# ---- gated_residual_norm: generic and mode-specialised -------------------------------------------------------------------------------------
def _grn_name(d, post_mode, next_mode, spec):
    n = ((d >> 3) + 63) // 64
    if spec and next_mode in (1, 2) and n in (3, 5, 6):
        return f"gated_residual_norm_kernel<{n},{post_mode},0,{next_mode}>"
    return f"gated_residual_norm_kernel<{R.maxch(d)}>"


# (d, post_mode, next_mode, norm_specialize, apex, h_pair)
GRN_CASES = [(d, pm, nm, sp, 0, 0) for d in (576, 1536) for pm in (0, 1) for nm in (0, 1, 2) for sp in (0, 1)]
GRN_CASES += [(d, 1, nm, sp, 0, 0) for d in (2304, 3072) for nm in (1, 2) for sp in (0, 1)]
GRN_CASES += [(d, pm, nm, 1, 0, 0) for d in (2304, 3072) for pm in (0,) for nm in (1, 2)]
GRN_CASES += [(d, 1, nm, 1, 0, 0) for d in (8, 520, 4096) for nm in (1, 2)]
GRN_CASES += [(d, 1, 1, 1, 1, 0) for d in (576, 2304)] + [(576, 1, 2, 1, 1, 0)]          # option rmsnorm_apex: the generic kernel
GRN_CASES += [(d, 1, 1, sp, 0, 1) for d, sp in ((576, 1), (2304, 0), (2304, 1))]          # h in the pair layout


def _grn_run(b, x, y, pw, gate_i, mod, ld, d, B, N, post_mode, next_mode, nw, ns_i, nsh_i, h_pair=0, ystat=None, moe=None, route=None):
    """one launch; -> (x' device view, h device view or None, route outputs)"""
    xd, yd, pwd, md, nwd = b.put(x), b.put(y), b.put(pw), b.put(mod), b.put(nw)
    h = b.out(B * N, d) if next_mode else None
    ysd = b.put(ystat)
    mo = [b.put(t) for t in moe] if moe else [None, None, None]
    rw, E, forced = route if route else (None, 0, None)
    rwd, fd = b.put(rw), b.put(forced)
    sel = b.out(B * N, 2, dtype=torch.int32, fill=-1) if rw is not None else None
    wts = b.out(B * N, 2) if rw is not None else None
    if wts is not None and moe:
        wts.copy_(mo[2])           # (the engine routes into the buffer the combine weights came from: the kernel reads them first)
        mo[2] = wts
    ok(lib().lt_op_gated_residual_norm_ex(P(xd), P(yd), P(pwd) if post_mode else None, _sub(md, gate_i, d), post_mode, 0, P(nwd) if next_mode == 1 else None,
                                          _sub(md, ns_i, d) if next_mode and ns_i is not None else None,
                                          _sub(md, nsh_i, d) if next_mode and nsh_i is not None else None, next_mode, ld, P(h), B, N, d, EPS, EPS2, 1,
                                          h_pair, P(ysd), ystat.shape[1] if ystat is not None else 0, P(mo[0]), P(mo[1]), P(mo[2]), P(rwd), E, P(sel), P(wts),
                                          P(fd), stream()), "gated_residual_norm")
    return xd, h, sel, wts


@pytest.mark.parametrize("d,post_mode,next_mode,spec,apex,h_pair", GRN_CASES)
def test_gated_residual_norm_is_word_exact(d, post_mode, next_mode, spec, apex, h_pair):
    B, N = (2, 7) if h_pair else (3, 5)
    x, y = R.draw_rows(B * N, d, d + 1, std=1.0, mean_rows=True), R.draw_rows(B * N, d, d + 2, std=2.0)
    pw, nw = R.draw_vec(d, d + 3, 1.0), R.draw_vec(d, d + 4, 1.0)
    mod, ld, (gate, ns, nsh) = _mod(B, d, 3, d + 5)
    mod[:, OFF + d:OFF + 2 * d] = (1.0 + ns.float()).to(torch.bfloat16)      # prepared: bf16(1 + scale)
    has_shift = next_mode == 2 or d == 576
    set_option("norm_specialize", spec)
    set_option("rmsnorm_apex", apex)
    kernel = _grn_name(d, post_mode, next_mode, spec and not apex)
    assert _describe(post_mode, next_mode, d, next_mode == 1, next_mode != 0, next_mode != 0 and has_shift, 1) == kernel
    what = f"{kernel} d {d} post {post_mode} next {next_mode} apex {apex} h_pair {h_pair}"
    b = Bufs()
    xd, h, _, _ = _grn_run(b, x, y, pw, 0, mod, ld, d, B, N, post_mode, next_mode, nw, 1, 2 if has_shift else None, h_pair)
    b.done(what)
    share = R.assert_row_words(xd, R.ref_gated_x(x, y, pw, gate, B, N, EPS, post_mode, apex), what + " x'", N=N)
    if next_mode:
        hg = R.from_pair(h.cpu(), B * N, d) if h_pair else h
        ch = R.ref_gated_h(xd, nw if next_mode == 1 else None, ns, nsh if has_shift else None, B, N, EPS, EPS2, next_mode, 1, apex)
        share = max(share, R.assert_row_words(hg, ch, what + " h", N=N))
    _report(kernel, what, share)


# ---- the streaming kernel on test-made partials ----------------------------------------------------------------------------------------------
def _partials(y, slots, seed):
    """[rows, slots] fp32: sums of squares over `slots` unequal column ranges (the kernel must add exactly what it is given)"""
    d = y.shape[1]
    g = torch.Generator().manual_seed(seed)
    cuts = sorted(torch.randperm(d - 1, generator=g)[:slots - 1].add(1).tolist())
    edges = [0] + cuts + [d]
    sq = y.double() ** 2
    return torch.stack([sq[:, edges[s]:edges[s + 1]].sum(-1) for s in range(slots)], -1).float()


@pytest.mark.parametrize("h_pair", [0, 1])
@pytest.mark.parametrize("slots", [12, 18])
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("d", [1536, 2304])
def test_streaming_gated_residual_norm_on_given_partials_is_word_exact(d, form, slots, h_pair):
    B, N = (2, 7) if h_pair else (3, 5)           # 15 rows: the last wave of the two-rows-per-wave form holds one row
    x, y = R.draw_rows(B * N, d, d + 11, std=1.0), R.draw_rows(B * N, d, d + 12, std=2.0)
    pw, nw = R.draw_vec(d, d + 13, 1.0), R.draw_vec(d, d + 14, 1.0)
    mod, ld, (gate, ns) = _mod(B, d, 2, d + 15)
    ns = (1.0 + ns.float()).to(torch.bfloat16)
    mod[:, OFF + d:OFF + 2 * d] = ns
    ystat = _partials(y, slots, d + slots)
    set_option("grn_ystat", form)
    kernel = f"gated_residual_norm_ys_kernel<{d // 256},{form}>"
    assert _describe(1, 1, d, 1, 1, 0, 1, ystat_slots=slots) == kernel
    what = f"{kernel} slots {slots} h_pair {h_pair}"
    b = Bufs()
    xd, h, _, _ = _grn_run(b, x, y, pw, 0, mod, ld, d, B, N, 1, 1, nw, 1, None, h_pair, ystat=ystat)
    b.done(what)
    share = R.assert_row_words(xd, R.ref_gated_x(x, y, pw, gate, B, N, EPS, 1, 0, ystat), what + " x'", N=N)
    hg = R.from_pair(h.cpu(), B * N, d) if h_pair else h
    share = max(share, R.assert_row_words(hg, R.ref_gated_h(xd, nw, ns, None, B, N, EPS, EPS2, 1), what + " h", N=N))
    _report(kernel, what, share)


# ---- MoE combine-on-load, routing on the way out ---------------------------------------------------------------------------------------------
def _moe_inputs(rows, d, seed):
    g = torch.Generator().manual_seed(seed)
    nsorted = 2 * rows + 9
    ys = R.draw_rows(nsorted, d, seed, std=2.0)
    pos = torch.randperm(nsorted, generator=g)[:2 * rows].view(rows, 2).int()        # a permutation with padding gaps
    wa = torch.rand(rows, 1, generator=g) * 0.6 + 0.2
    return ys, pos, torch.cat([wa, 1 - wa], 1).to(torch.bfloat16)


# (d, next_mode, route E (0: no routing), forced)
MOE_CASES = [(1536, 1, 0, 0), (1536, 2, 0, 0), (2048, 1, 0, 0), (2048, 2, 0, 0)]
MOE_CASES += [(d, 1, E, f) for d in (1536, 2048) for E, f in ((2, 0), (R.LT_MOE_MAX_E, 0), (R.LT_MOE_MAX_E, 1))]      # (LT_MOE_MAX_E is 8)
MOE_CASES += [(1536, 1, 5, 0)]


@pytest.mark.parametrize("d,next_mode,E,forced", MOE_CASES)
def test_moe_combine_on_load_and_routing_are_word_exact(d, next_mode, E, forced):
    B, N = 3, 5
    rows = B * N
    x = R.draw_rows(rows, d, d + 21, std=1.0, mean_rows=True)
    ys, pos, cw = _moe_inputs(rows, d, d + 22)
    pw, nw = R.draw_vec(d, d + 23, 1.0), R.draw_vec(d, d + 24, 1.0)
    mod, ld, (gate, ns, nsh) = _mod(B, d, 3, d + 25)
    ns = (1.0 + ns.float()).to(torch.bfloat16)
    mod[:, OFF + d:OFF + 2 * d] = ns
    has_shift = next_mode == 2
    rw = R.draw_vec(E * d, d + 26, 0.0, 0.05).view(E, d) if E else None
    fz = None
    if forced:
        g = torch.Generator().manual_seed(d)
        fz = torch.stack([torch.randperm(E, generator=g)[:2] for _ in range(rows)]).int()       # both orders occur
    kernel = f"gated_residual_norm_kernel<3,1,0,{next_mode},moe>" if d == 1536 else "gated_residual_norm_kernel<4,-1,-1,-1,moe>"
    assert _describe(1, next_mode, d, next_mode == 1, 1, has_shift, 1, moe=1) == kernel
    what = f"{kernel} d {d} next {next_mode} route E {E} forced {forced}"
    b = Bufs()
    xd, h, sel, wts = _grn_run(b, x, None, pw, 0, mod, ld, d, B, N, 1, next_mode, nw, 1, 2 if has_shift else None, moe=(ys, pos, cw),
                               route=(rw, E, fz) if E else None)
    b.done(what)
    y = R.moe_combine(ys, pos, cw).to(torch.bfloat16)
    share = R.assert_row_words(xd, R.ref_gated_x(x, y, pw, gate, B, N, EPS), what + " x'", N=N)
    ch = R.ref_gated_h(xd, nw if next_mode == 1 else None, ns, nsh if has_shift else None, B, N, EPS, EPS2, next_mode)
    share = max(share, R.assert_row_words(h, ch, what + " h", N=N))
    if E:
        namb = R.check_routing(h, rw, sel, wts, fz, what)
        print(f"ROWS routing rows_with_ambiguous_logit={namb} of {rows}")
    _report(kernel, what, share)


# ---- lt_op_prep_mod ----------------------------------------------------------------------------------------------------------------------------
def test_prep_mod_is_word_exact():
    """chunk 1 -> bf16(tanh(gate)), chunk 2 -> bf16(1 + scale), chunks 0 and 3 and the padding columns untouched (in place, two layers)"""
    B, L, chunks, d = 3, 2, 4, 520
    ld = L * chunks * d + 40
    mod = R.draw_mod(B, ld, 31, std=1.0)
    b = Bufs()
    md = b.put(mod)
    ok(lib().lt_op_prep_mod(P(md), B, ld, L, chunks, d, 0b0010, 0b0100, -1, stream()))
    b.done("prep_mod")
    got, src = md.cpu().view(B, ld), mod.double()
    body = lambda t: t[:, :L * chunks * d].reshape(B, L, chunks, d)
    g4, s4 = body(got), body(src)
    assert torch.equal(g4[:, :, 0], body(mod)[:, :, 0]) and torch.equal(g4[:, :, 3], body(mod)[:, :, 3]) and torch.equal(got[:, L * chunks * d:], mod[:, L * chunks * d:])
    tanh = R.Chain((B * L, d)).round(lambda _: torch.tanh(s4[:, :, 1]).reshape(B * L, d), rel=R.DELTA_TANH)
    share = R.assert_row_words(g4[:, :, 1].reshape(B * L, d), tanh, "prep_mod tanh")
    one = R.Chain((B * L, d)).round(lambda _: 1.0 + s4[:, :, 2].reshape(B * L, d), sum2=True)
    R.assert_row_words(g4[:, :, 2].reshape(B * L, d), one, "prep_mod 1 + scale")
    _report("prep_mod_kernel", "tanh / 1 + scale", share)


# ---- qk_norm_rope: persistent, pair and fused forms; the V image ----------------------------------------------------------------------------
WATERSHED = 0.3
# (heads, kv_heads, hd, qk_norm, rope_mode, k out_scale, grid (N = h x w or (N, w)), t, packed)
QK_BASE = dict(qk_norm=1, rope_mode=1, osc=0.1875, N=60, gw=10, t=0.9, packed=0)
QK_CASES = [dict(QK_BASE, heads=h, kvh=k, hd=hd) for h, k, hd in [(2, 1, 72), (8, 8, 72), (32, 8, 72), (32, 32, 48), (16, 4, 96), (32, 32, 128)]]
QK_CASES += [dict(QK_BASE, heads=8, kvh=2, hd=72, **kw) for kw in [dict(qk_norm=0), dict(rope_mode=0), dict(rope_mode=2), dict(rope_mode=0, qk_norm=0, osc=1.0),
                                                                  dict(N=13, gw=5), dict(t=0.1), dict(packed=1), dict(packed=1, rope_mode=2, t=None), dict(osc=1.0)]]
QK_CASES += [dict(QK_BASE, heads=32, kvh=8, hd=128, rope_mode=2, N=13, gw=13), dict(QK_BASE, heads=32, kvh=32, hd=48, qk_norm=0, N=13, gw=4, t=0.1)]


@pytest.mark.parametrize("c", QK_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if k in ("heads", "kvh", "hd") or QK_BASE.get(k) != v))
def test_qk_norm_rope_forms_are_word_exact(c):
    """q (out_scale 1) and k (GQA width, non-trivial out_scale) of one projection output through the persistent kernel (one launch each), the
    q + k pair launch and the fused q / k / V launch: each output against the float64 chain; the fused launch's V image bit for bit"""
    heads, kvh, hd, N, gw = c["heads"], c["kvh"], c["hd"], c["N"], c["gw"]
    B, mode = 2, c["rope_mode"]
    rows, wq, wk = B * N, heads * hd, kvh * hd
    ld, q0 = 64 + wq + 2 * wk + 8, 64
    k0, v0 = q0 + wq, q0 + wq + wk
    qkv = R.draw_rows(rows, ld, wq + hd + N, std=1.0, mean_rows=True)
    ln = [(R.draw_vec(w, w + i, 1.0), R.draw_vec(w, w + i + 1, 0.0)) if c["qk_norm"] else (None, None) for i, w in ((0, wq), (2, wk))]
    cs_len = 64
    table = R.rope_table(cs_len, hd // 4 if mode == 1 else max(hd // 2, 1))
    branch = 1 if c["t"] is None or not (R.f32(c["t"]) < R.f32(WATERSHED)) else 0
    ntok, gwb = (torch.tensor([N, 35], dtype=torch.int32), torch.tensor([gw, 7], dtype=torch.int32)) if c["packed"] else (None, None)
    Npad = (N + 63) // 64 * 64
    assert N % 64 != 0
    refs = [R.ref_qk_norm_rope(qkv, col, w_, b_, EPS, B, N, hh, hd, mode, table, branch, gw, osc, ntok, gwb)
            for col, (w_, b_), hh, osc in ((q0, ln[0], heads, 1.0), (k0, ln[1], kvh, c["osc"]))]
    want_v = R.v_image(qkv, v0, B, N, Npad, kvh, hd)
    b = Bufs()
    src, tb = b.put(qkv), b.put(table)
    lnd = [(b.put(w_), b.put(b_)) for w_, b_ in ln]
    td = b.put(torch.tensor([c["t"], 0.0], dtype=torch.float32)) if c["t"] is not None else None
    nt, gb = b.put(ntok), b.put(gwb)
    common = (mode, P(tb), cs_len, P(td), WATERSHED, gw, P(nt), P(gb))
    outs = {}
    q1, k1 = b.out(B, heads, N, hd), b.out(B, kvh, N, hd)
    ok(lib().lt_op_qk_norm_rope_ex(P(src), ld, q0, P(lnd[0][0]), P(lnd[0][1]), EPS, P(q1), B, N, heads, hd, *common, 1.0, None, None, 0, 0, stream()), "persistent q")
    ok(lib().lt_op_qk_norm_rope_ex(P(src), ld, k0, P(lnd[1][0]), P(lnd[1][1]), EPS, P(k1), B, N, kvh, hd, *common, c["osc"], None, None, 0, 0, stream()), "persistent k")
    outs["persistent"] = (q1, k1)
    q2, k2 = b.out(B, heads, N, hd), b.out(B, kvh, N, hd)
    ok(lib().lt_op_qk_norm_rope_pair(P(src), ld, q0, k0, P(lnd[0][0]), P(lnd[0][1]), P(lnd[1][0]), P(lnd[1][1]), EPS, P(q2), P(k2), B, N, heads, kvh, hd, *common,
                                     1.0, c["osc"], stream()), "pair")
    outs["pair"] = (q2, k2)
    q3, k3, vt = b.out(B, heads, N, hd), b.out(B, kvh, N, hd), b.out(B, kvh, hd, Npad)
    ok(lib().lt_op_qkv_post(P(src), ld, q0, k0, v0, P(lnd[0][0]), P(lnd[0][1]), P(lnd[1][0]), P(lnd[1][1]), EPS, P(q3), P(k3), P(vt), B, N, Npad, heads, kvh, hd,
                            *common, 1.0, c["osc"], stream()), "qkv_post")
    outs["fused"] = (q3, k3)
    what = f"qk_norm_rope {c}"
    b.done(what)
    assert torch.equal(src.cpu(), qkv)
    for form, (qd, kd) in outs.items():
        sq = R.assert_row_words(R.head_major(qd.cpu(), B, N, heads, hd), refs[0], f"{what} {form} q", N=N, hd=hd)
        sk = R.assert_row_words(R.head_major(kd.cpu(), B, N, kvh, hd), refs[1], f"{what} {form} k", N=N, hd=hd)
        _report(f"qk_norm_rope[{form}]<{R.maxch(wq)}>", what, max(sq, sk))
    assert torch.equal(vt.cpu().view(torch.int16), want_v.view(torch.int16)), "V image of lt_op_qkv_post"


@pytest.mark.parametrize("slots,width", [(8, 2304), (16, 2304), (3, 576)])
def test_qstat_reduction_is_within_the_statistics_bound(slots, width):
    """the K pass reduces given (sum, sum of squares) partials of Q's rows to (mean, rstd): against float64 from the same partials"""
    B, N, heads, hd = 3, 5, 2, 72
    rows = B * N
    q = R.draw_rows(rows, width, width + slots, std=1.0, mean_rows=True).double()
    edges = [width * s // slots for s in range(slots + 1)]
    part = torch.stack([torch.stack([q[:, edges[s]:edges[s + 1]].sum(-1), (q[:, edges[s]:edges[s + 1]] ** 2).sum(-1)], -1) for s in range(slots)], 1).float()
    src, w_, b_ = R.draw_rows(rows, heads * hd, 41, std=1.0), R.draw_vec(heads * hd, 42, 1.0), R.draw_vec(heads * hd, 43)
    table = R.rope_table(64, hd // 4)
    b = Bufs()
    sd, wd, bd, tb, pd = b.put(src), b.put(w_), b.put(b_), b.put(table), b.put(part)
    dst, so = b.out(B, heads, N, hd), b.out(rows, 2, dtype=torch.float32)
    ok(lib().lt_op_qk_norm_rope_ex(P(sd), heads * hd, 0, P(wd), P(bd), EPS, P(dst), B, N, heads, hd, 1, P(tb), 64, None, 0.0, 5, None, None, 1.0, P(pd), P(so),
                                   slots, width, stream()), "qstat")
    b.done("qstat")
    mean, rstd, mb, rb = R.ref_qstat(part, width, EPS)
    got = so.cpu().double()
    em, er = (got[:, 0] - mean).abs(), (got[:, 1] - rstd).abs()
    print(f"ROWS qstat slots {slots} width {width}: worst mean error / bound {float((em / mb).max()):.3f}, rstd {float((er / rb).max()):.3f}")
    assert bool((em <= mb).all()) and bool((er <= rb).all()), (em / mb, er / rb)
    share = R.assert_row_words(R.head_major(dst.cpu(), B, N, heads, hd), R.ref_qk_norm_rope(src, 0, w_, b_, EPS, B, N, heads, hd, 1, table, 1, 5), "qstat pass k", N=N, hd=hd)
    _report("qk_norm_rope[persistent+qstat]", f"slots {slots} width {width}", share)
