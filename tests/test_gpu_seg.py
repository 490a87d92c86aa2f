"""GPU: smoothed-energy guidance - lt_op_query_blur / lt_forward_blur / lt_forward_cfg_seg / lt_sample_ode_cfg_seg.

* kernel: exact operands word for word; Gaussian taps against the float64 chain of tests/exact_seg.py under the rule of test_gpu_rows_exact.py
  (RN_bf16(ref); the range RN(ref - bound) .. RN(ref + bound) of the derived fp32 bound, i.e. the neighbour only near a bf16 midpoint, and
  more only on the words that cancel below the bound - exact_seg.check_words; one run's shares: profiles/seg/); mean mode word for word; NaN-filled guarded outputs,
  source words unchanged, the refusals by name;
* engine: a blur whose taps are (0, 1, 0) is the unblurred model on the blurred block's launch route; sigma moves the words; the plans agree
  (small_fused on / off, pair_layout 1 / 0); the guided call equals the host expressions; the engine's trajectory equals
  ``transport.guidance.sample_cfg_seg`` state for state; graph keys; no set is left behind; the refusals by name."""
import math

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

import exact_rows as R
import exact_seg as XS
from gpu_util import P, lib, stream
from test_gpu_caller_capture import KW_BIG, _new_engine
from test_gpu_slg import DTYPES, STEP_KW, _build, _counts, _deep, _grid, _mixed

pytestmark = pytest.mark.gpu

SHARES = {}     # case -> share of the words that used the midpoint allowance (printed; profiles/seg/ keeps one run's figures)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run_kernel(q, grid_w, blur_w, taps, mode):
    L = lib()
    B, H, N, hd = q.shape
    kept = q.clone()
    buf = R.GuardedBuf(q.numel())
    tp = None if taps is None else torch.tensor(list(taps), dtype=torch.float32, device="cuda")
    r = 0 if taps is None else (len(taps) - 1) // 2
    rc = L.lt_op_query_blur(P(q), P(buf.out), None if tp is None else P(tp), B, H, N, hd, grid_w, blur_w, r, mode, stream())
    assert rc == 0, L.lt_last_error()
    torch.cuda.synchronize()
    buf.assert_intact(f"query_blur {tuple(q.shape)} grid_w {grid_w} blur_w {blur_w} r {r} mode {mode}")
    assert torch.equal(_bits(q), _bits(kept)), "the source words changed"
    return buf.out.view(q.shape)


def _ints(B, H, Hp, grid_w, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (B, H, Hp * grid_w, hd), generator=g).to("cuda", torch.bfloat16)


def _randn(B, H, Hp, grid_w, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, Hp * grid_w, hd, generator=g).mul(3).to("cuda", torch.bfloat16)


# (B, H, Hp, grid_w, blur_w, hd, r): the issue's grids, an end-of-line grid, one taller than a strip of 32 rows (three strips, the last partial),
# one wider than a tile of 16 columns, and one of 1152 work items - beyond a pass of the grid capped at 1024 blocks
SHAPES = [(1, 2, 2, 2, 2, 48, 1), (3, 2, 4, 4, 4, 72, 3), (1, 4, 5, 9, 9, 96, 4), (1, 2, 9, 5, 5, 128, 4), (1, 2, 33, 32, 32, 72, 31),
          (3, 4, 6, 8, 7, 96, 2), (1, 2, 70, 5, 5, 48, 3), (3, 4, 40, 40, 40, 128, 2)]
IDS = ["2x2", "4x4", "5x9", "9x5", "33x32_r31", "eol", "tall", "beyond_cap"]


@pytest.mark.parametrize("taps", [(1, 2, 1), (1, 4, 6, 4, 1)], ids=["121", "14641"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if min(s[2], s[4]) >= 3], ids=[i for s, i in zip(SHAPES, IDS) if min(s[2], s[4]) >= 3])
def test_kernel_exact_operands_word_for_word(shape, taps):
    B, H, Hp, grid_w, blur_w, hd, _ = shape
    w = [v / float(sum(taps)) for v in taps]
    q = _ints(B, H, Hp, grid_w, hd, 7 * Hp + grid_w)
    got = _run_kernel(q, grid_w, blur_w, w, 0)
    want = XS.rn_bf16(XS.blur_ref(q.cpu(), grid_w, blur_w, w)).to(torch.bfloat16)
    bad = _bits(got.cpu()) != _bits(want)
    assert not bool(bad.any()), (shape, taps, int(bad.sum()), bad.nonzero()[0].tolist())


def test_kernel_exact_operands_on_the_two_by_two_grid():
    q = _ints(1, 2, 2, 2, 48, 5)
    w = [0.25, 0.5, 0.25]
    got = _run_kernel(q, 2, 2, w, 0)
    assert torch.equal(_bits(got.cpu()), _bits(XS.rn_bf16(XS.blur_ref(q.cpu(), 2, 2, w)).to(torch.bfloat16)))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernel_gaussian_taps_against_the_float64_chain(shape):
    B, H, Hp, grid_w, blur_w, hd, r = shape
    mode, rr, taps = G.seg_taps((r - 0.5) / 3.0)
    assert mode == 0 and rr == r
    q = _randn(B, H, Hp, grid_w, hd, 11 * Hp + grid_w + hd)
    got = _run_kernel(q, grid_w, blur_w, taps.tolist(), 0)
    t64 = taps.double().tolist()
    share = XS.check_words(got, XS.blur_ref(q.cpu(), grid_w, blur_w, t64), XS.blur_bound(q.cpu(), grid_w, blur_w, t64), str(shape))
    SHARES[shape] = share
    print(f"query_blur {shape}: {share:.4%} of the words used the midpoint allowance")
    assert share < 0.02


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[5], SHAPES[6]], ids=["4x4", "33x32", "eol", "tall"])
def test_kernel_mean_mode_word_for_word(shape):
    B, H, Hp, grid_w, blur_w, hd, _ = shape
    q = _randn(B, H, Hp, grid_w, hd, 13 * Hp + grid_w)
    got = _run_kernel(q, grid_w, blur_w, None, 1)
    want = XS.rn_bf16(XS.mean_ref(q.cpu(), grid_w, blur_w)).to(torch.bfloat16)
    bad = _bits(got.cpu()) != _bits(want)
    assert not bool(bad.any()), (shape, int(bad.sum()))


def test_kernel_refusals_by_name():
    L = lib()
    q = torch.zeros(2 * 2 * 64 * 48 + 8, dtype=torch.bfloat16, device="cuda")
    out = torch.full((2 * 2 * 64 * 48 + 8,), float("nan"), dtype=torch.bfloat16, device="cuda")
    taps = torch.full((64,), 1.0 / 3, dtype=torch.float32, device="cuda")

    def call(s=q, o=out, tp=taps, B=2, H=2, N=64, hd=48, grid_w=8, blur_w=8, r=1, mode=0):
        return L.lt_op_query_blur(None if s is None else P(s), None if o is None else P(o), None if tp is None else P(tp), B, H, N, hd, grid_w, blur_w,
                                  r, mode, stream())

    for kw, word in ((dict(s=None), "null argument"), (dict(o=None), "null argument"), (dict(tp=None), "null argument"), (dict(hd=64), "head_dim 64 not built"),
                     (dict(grid_w=7), "not a whole number of grid rows"), (dict(blur_w=0), "blur_w=0 outside"), (dict(blur_w=9), "blur_w=9 outside"),
                     (dict(r=-1), "radius -1 outside"), (dict(r=32), "radius 32 outside"), (dict(r=8), "cannot be reflected"),
                     (dict(grid_w=16, blur_w=16, r=4), "cannot be reflected"), (dict(o=out[1:]), "not aligned"), (dict(s=q[1:]), "not aligned"),
                     (dict(o=q), "q == out"), (dict(mode=2), "mode 2"), (dict(B=0), "bad shape")):
        rc = call(**kw)
        msg = L.lt_last_error().decode()
        assert rc != 0 and "query_blur" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0 and call(tp=None, mode=1, r=0) == 0, L.lt_last_error()


# ---- engine ------------------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _family(golden_dir, fam):
    if fam not in _MODELS:
        cfg, sd, cond = _deep(golden_dir, fam)
        _MODELS[fam] = (_build(fam, cfg, sd), cond)
    return _MODELS[fam]


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


@pytest.mark.parametrize("fam", ["next", "imagenet", "flag"])
def test_blurred_forward_identity_taps_sigma_and_sets(golden_dir, fam):
    model, cond = _family(golden_dir, fam)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(21)).to("cuda", torch.bfloat16)
    t = torch.full((1,), 0.4, device="cuda")
    half = tuple(c[:1].contiguous() for c in cond)
    if fam != "imagenet":
        model.forward_with_cfg(torch.cat([z, z]), torch.cat([t, t]), *cond, 4.0, **STEP_KW)  # the flags a plain forward reads
    plain = model.forward(z, t, *half).clone()
    # sigma 0.05: radius 1, taps (0, 1, 0) exactly - the blurred block is the block, on its own launch route (a bf16 network's rounding apart)
    assert G.seg_taps(0.05)[2].tolist() == [0.0, 1.0, 0.0]
    ident = model.forward(z, t, *half, blur_layers=[0, 1, 2, 3], blur_sigma=0.05)
    assert _rel(ident, plain) < 2e-2, (fam, _rel(ident, plain))
    outs = {}
    for sigma in (1.0, 2.0, math.inf):
        o = model.forward(z, t, *half, blur_layers=[3, 1], blur_sigma=sigma).clone()
        assert bool(torch.isfinite(o.float()).all()) and not torch.equal(o, plain), (fam, sigma)
        assert torch.equal(model.forward(z, t, *half, blur_layers=[1, 3], blur_sigma=sigma), o), (fam, sigma, "order of the set / repeat of the call")
        assert torch.equal(model.forward(z, t, *half), plain), (fam, sigma, "a set was left behind")
        outs[sigma] = o
    assert not torch.equal(outs[1.0], outs[2.0]) and not torch.equal(outs[2.0], outs[math.inf])
    assert _rel(outs[1.0], plain) < _rel(outs[math.inf], plain) * 1.5      # (a wider blur is no smaller a perturbation, loosely)
    both = model.forward(z, t, *half, blur_layers=[1], skip_layers=[2], blur_sigma=1.0)
    assert not torch.equal(both, model.forward(z, t, *half, skip_layers=[2])) and not torch.equal(both, model.forward(z, t, *half, blur_layers=[1], blur_sigma=1.0))


def test_blurred_forward_is_the_same_with_the_small_fused_route_off(golden_dir):
    model, (y,) = _family(golden_dir, "imagenet")
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(22)).to("cuda", torch.bfloat16)
    t = torch.full((2,), 0.3, device="cuda")
    # every block blurred: none runs the one-launch attention, whose words are its own - what is left is the blurred block's route, twice
    on = model.forward(z, t, y, blur_layers=[0, 1, 2, 3], blur_sigma=1.5).clone()
    model._engine.set_option("attn_small_fused", 0)
    try:
        off = model.forward(z, t, y, blur_layers=[0, 1, 2, 3], blur_sigma=1.5)
    finally:
        model._engine.set_option("attn_small_fused", None)
    assert torch.equal(on, off), int((on != off).sum())


def test_pair_plan_blurred_forward_equals_the_row_major_plan():
    cfg = synth.NextDiTConfig(n_layers=2)
    sd = {k: v.to("cuda", torch.bfloat16) for k, v in synth.synth_state_dict(cfg, seed=81).items()}
    z, t, cap, mask = synth.synth_inputs(cfg, latent_hw=(128, 128), text_len=128, uncond_len=8, seed=82)
    z, t, cap, mask = z.to("cuda", torch.bfloat16), t.cuda().float(), cap.to("cuda", torch.bfloat16), mask.to("cuda", torch.int32)
    kw = dict(base_seqlen=KW_BIG["base_seqlen"], proportional_attn=True)
    eng = _new_engine(cfg, sd, graph=0)
    eng.prepare_prompt(cap, mask)
    res = {}
    for pair in (1, 0, 1):
        eng.set_option("pair_layout", pair)
        before = eng.forward(z, t, use_cfg=False, **kw).clone()
        assert eng.get_option("last_pair") == pair
        got = eng.forward(z, t, use_cfg=False, blur_layers=[1], blur_sigma=10.0, **kw).clone()
        assert eng.get_option("last_pair") == pair
        assert torch.equal(eng.forward(z, t, use_cfg=False, **kw), before), pair
        assert bool(torch.isfinite(got.float()).all()) and not torch.equal(got, before)
        for name, v in (("plain", before), ("blurred", got)):
            if name in res:
                assert torch.equal(v, res[name]), (name, pair, int((v != res[name]).sum()))
            res[name] = v
    eng.set_option("pair_layout", None)


def test_forward_with_cfg_seg_equals_the_host_expressions(golden_dir):
    model, (cap, cmask) = _family(golden_dir, "next")
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(12)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    t = torch.full((2,), 0.25, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    assert torch.equal(model.forward_with_cfg_seg(z, t, cap, cmask, 4.0, seg_scale=0.0, seg_layers=[1], seg_sigma=2.0, **STEP_KW), ref)
    got = model.forward_with_cfg_seg(z, t, cap, cmask, 4.0, seg_scale=2.8, seg_layers=[1, 3], seg_sigma=2.0, skip_layers=[2], **STEP_KW)
    got1 = model.forward_with_cfg_seg(z, t, cap, cmask, 1.0, seg_scale=-1.5, seg_layers=[1, 3], seg_sigma=math.inf, **STEP_KW)
    o = model.forward(z, t, cap, cmask).to(torch.bfloat16)
    half = (z[:1], t[:1], cap[:1].contiguous(), cmask[:1].contiguous())
    k = model.forward(*half, skip_layers=[2], blur_layers=[1, 3], blur_sigma=2.0)
    k1 = model.forward(*half, blur_layers=[1, 3], blur_sigma=math.inf)
    c, u = o[:1, :3], o[1:, :3]
    gch = G.slg_combine(c, u, k[:, :3], 4.0, 2.8)
    assert torch.equal(got, torch.cat([torch.cat([gch, gch]), o[:, 3:]], 1)) and not torch.equal(got, ref)
    r = torch.cat([G.slg_combine(c, None, k1[:, :3], 1.0, -1.5), o[:1, 3:]], 1)
    assert torch.equal(got1, torch.cat([r, r]))
    model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, (cap, cmask) = _family(golden_dir, "next")
    tgrid = _grid(method)
    w, s = _mixed(method)      # guided, conditional-only, s != 0 at w != 1 and s != 0 at w == 1; zeros in s
    nfe, rows1 = _counts(w, s)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(6)).to("cuda", dtype).repeat(2, 1, 1, 1)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), cap, cmask, 4.0, **STEP_KW)
    run = lambda **kw: model.sample_ode_cfg_schedule(z, tgrid, w, cap, cmask, method=method, return_trajectory=True, **kw, **STEP_KW)
    slg_only = run(slg=s, slg_layers=[1])
    for ql, sl, sigma in (([2, 0], [1], 1.5), ([0, 1, 2, 3], [], math.inf)):
        tag = (method, dtype, tuple(ql), tuple(sl), sigma)
        got = run(seg=s, seg_layers=ql, seg_sigma=sigma, slg_layers=sl)
        eng = model._engine
        assert eng.last_nfe() == nfe and eng.last_eval_rows() == rows1, tag + (eng.last_nfe(), eng.last_eval_rows())
        want = G.sample_cfg_seg(model, z, tgrid, w, s, ql, sigma, sl, method, cap_feats=cap, cap_mask=cmask, **STEP_KW)
        assert got.shape == want.shape == (len(tgrid),) + tuple(z.shape) and got.dtype == dtype and bool(torch.isfinite(want.float()).all()), tag
        for i in range(len(tgrid)):
            assert torch.equal(got[i], want[i]), tag + (i, int((got[i] != want[i]).sum()))
        assert not torch.equal(got[-1], slg_only[-1]), tag
    # an interval table; Q empty: skip-layer guidance; every s == 0: the schedule call
    si = G.seg_table(tgrid, method, 2.0, (0.3, 0.8))
    assert 0 < int((si != 0).sum()) < si.numel()
    got = run(seg=si, seg_layers=[1], seg_sigma=1.0)
    assert torch.equal(got, G.sample_cfg_seg(model, z, tgrid, w, si, [1], 1.0, (), method, cap_feats=cap, cap_mask=cmask, **STEP_KW))
    assert torch.equal(run(seg=s, seg_layers=[], seg_sigma=1.0, slg_layers=[1]), slg_only)
    assert torch.equal(run(seg=torch.zeros_like(s), seg_layers=[1], seg_sigma=1.0), run())


def test_graph_keys_sigma_at_equal_radius_and_no_set_left_behind(golden_dir):
    cfg, sd, (cap, cmask) = _deep(golden_dir, "next")
    model = _build("next", cfg, sd)  # a fresh engine: no key has been used
    H, W = 50, 82  # 25 x 41 = 1025 tokens: the smallest latent whose B' = 1 evaluation has more than 1024 rows
    tgrid = ODE(7, "midpoint", 4).t  # 12 stages
    w1 = torch.tensor([2.0, 3.0, 1.0, 3.5, 1.0, 1.0, 5.0, 2.0, 1.0, 1.0, 4.0, 3.0])
    s1 = torch.tensor([2.8, 0.0, 0.0, 1.5, 2.0, 0.0, 0.0, -1.0, 3.0, 0.0, 0.0, 0.5])
    z = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(8)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    t = torch.zeros(2, device="cuda")
    ref_cfg = model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW).clone()
    ref_plain = model.forward(z, t, cap, cmask).clone()
    model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW)
    eng = model._engine
    g, on = w1 != 1, s1 != 0
    k1 = [int((g & ~on).sum()), int((~g & ~on).sum()), int(on.sum()), int((g & on).sum()), int((~g & on).sum())]
    assert all(c > 0 for c in k1)
    run = lambda **kw: model.sample_ode_cfg_schedule(z, tgrid, w1, cap, cmask, method="midpoint", return_trajectory=True, seg=s1, **kw, **STEP_KW)
    before = eng.graph_replays()
    got = run(seg_layers=[1], seg_sigma=1.25, slg_layers=[2])      # radius 4
    assert eng.graph_replays() - before == sum(k1) - 5             # at most five keys: the first use of each runs eagerly
    mid = eng.graph_replays()
    other = run(seg_layers=[1], seg_sigma=1.3, slg_layers=[2])     # radius 4 again: the same five keys, every evaluation replays
    assert G.seg_taps(1.25)[1] == G.seg_taps(1.3)[1] == 4
    assert eng.graph_replays() - mid == sum(k1)
    assert not torch.equal(other, got)
    eng.set_option("graph", 0)
    try:
        assert torch.equal(run(seg_layers=[1], seg_sigma=1.25, slg_layers=[2]), got)
        assert torch.equal(run(seg_layers=[1], seg_sigma=1.3, slg_layers=[2]), other)
    finally:
        eng.set_option("graph", None)
    # blur {1}, perturb {1} and skip {1} are three keys: calls in alternation give their own words
    want = {"skip": model.forward(z, t, cap, cmask, skip_layers=[1]).clone(), "perturb": model.forward(z, t, cap, cmask, perturb_layers=[1]).clone(),
            "blur": model.forward(z, t, cap, cmask, blur_layers=[1], blur_sigma=1.25).clone()}
    assert len({tuple(v.view(-1)[:4096].tolist()) for v in want.values()} | {tuple(ref_plain.view(-1)[:4096].tolist())}) == 4
    mid = eng.graph_replays()
    for rep in range(2):
        assert torch.equal(model.forward(z, t, cap, cmask, skip_layers=[1]), want["skip"]), rep
        assert torch.equal(model.forward(z, t, cap, cmask, blur_layers=[1], blur_sigma=1.25), want["blur"]), rep
        assert torch.equal(model.forward(z, t, cap, cmask, perturb_layers=[1]), want["perturb"]), rep
        assert torch.equal(model.forward(z, t, cap, cmask), ref_plain), rep
    assert eng.graph_replays() - mid >= 6
    # a plain guided call, a PAG call and an SLG call before and after SEG calls give the words they gave alone
    pag = model.forward_with_cfg_pag(z, t, cap, cmask, 4.0, pag_scale=2.0, pag_layers=[1], **STEP_KW).clone()
    slg = model.forward_with_cfg_slg(z, t, cap, cmask, 4.0, slg_scale=2.0, slg_layers=[1], **STEP_KW).clone()
    seg = model.forward_with_cfg_seg(z, t, cap, cmask, 4.0, seg_scale=2.0, seg_layers=[1], seg_sigma=3.0, **STEP_KW).clone()
    assert not torch.equal(seg, pag) and not torch.equal(seg, slg)
    assert torch.equal(model.forward_with_cfg_pag(z, t, cap, cmask, 4.0, pag_scale=2.0, pag_layers=[1], **STEP_KW), pag)
    assert torch.equal(model.forward_with_cfg_slg(z, t, cap, cmask, 4.0, slg_scale=2.0, slg_layers=[1], **STEP_KW), slg)
    assert torch.equal(model.forward_with_cfg_seg(z, t, cap, cmask, 4.0, seg_scale=2.0, seg_layers=[1], seg_sigma=3.0, **STEP_KW), seg)
    # no set is left behind, also after refused calls; the outputs of a refused call stay untouched
    for bad, word in ((dict(seg_layers=[1, 1], seg_sigma=1.0), "repeated"), (dict(seg_layers=[9], seg_sigma=1.0), "outside"),
                      (dict(seg_layers=[1], slg_layers=[1], seg_sigma=1.0), "disjoint"), (dict(seg_layers=[1], seg_sigma=0.0), "not positive"),
                      (dict(seg_layers=[1], seg_sigma=-2.0), "not positive"), (dict(seg_layers=[], seg_sigma=1.0), "both layer sets are empty"),
                      (dict(seg_layers=[1], seg_sigma=1.0, pag=s1, pag_layers=[2]), "perturbed-attention"),
                      (dict(seg_layers=[1], seg_sigma=1.0, rescale=0.5), "rescale")):
        with pytest.raises((_lib.LuminaLibError, ValueError), match=word):
            run(**bad)
        assert torch.equal(model.forward(z, t, cap, cmask), ref_plain), bad
    zs = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(5)).to("cuda", torch.bfloat16)     # a 4 x 4 grid cannot reflect radius 4
    with pytest.raises(_lib.LuminaLibError, match="cannot be reflected"):
        model.forward(zs, t[:1], cap[:1].contiguous(), cmask[:1].contiguous(), blur_layers=[1], blur_sigma=1.25)
    with pytest.raises(_lib.LuminaLibError, match="perturb_layers"):
        model.forward(z, t, cap, cmask, blur_layers=[1], blur_sigma=1.0, perturb_layers=[2])
    with pytest.raises(_lib.LuminaLibError, match="blur_sigma"):
        model.forward(z, t, cap, cmask, blur_layers=[1])
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0, **STEP_KW), ref_cfg)
    assert torch.equal(model.forward(z, t, cap, cmask), ref_plain)
