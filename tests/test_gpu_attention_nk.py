"""-m gpu: per-sample key counts (AttnArgs::nk_batch) in the head_dim-72 one-wave kernel, through lt_op_attention_nk /
lt_op_attention_fused_nk: every output word against the float64 softmax of tests/exact_attention.py (DELTA, MAX_AMBIGUOUS unchanged) on
the cases of tests/attention_nk_cases.py - masked keys' K / V rows poisoned with finite words of magnitude 2^10, NaN-filled output
between sentinel guards - plus the pair-layout output, bit-identity with the ping-pong kernel on random operands, and the refusals."""
import pytest
import torch

import attention_nk_cases as K
import exact_attention as X
from exact_operands import Guarded
from gpu_util import P, lib, set_option, stream

pytestmark = pytest.mark.gpu

V4 = "attn_fwd_kernel_v4<72>"
_EXPECT = {}


@pytest.fixture(autouse=True)
def _variant_4():
    set_option("attention_variant", 4)
    yield
    set_option("attention_variant", 4)
    set_option("attn_text_skip", 1)


def _self(family, case):
    """(clean draw, poisoned k, poisoned v, float64 expectation) on the device, computed once per module and left unchanged"""
    key = (family, case)
    if key not in _EXPECT:
        inp = K.draw(family, *case, device="cuda")
        want = X.expected(inp)
        if family == "levels":
            assert all(s == 1.0 for s, n in zip(K.restricted_use(inp), case[4]) if n >= 2)
        _EXPECT[key] = (inp, *K.poison_masked(inp), want)
    return _EXPECT[key]


def test_dispatch_names_the_one_wave_kernel_with_key_counts():
    """fails without the feature: the hd-72 one-wave dispatch excluded nk_batch (and the entry did not exist)"""
    for B, H, Hkv, N in [(3, 2, 2, 320), (2, 8, 2, 128), (2, 32, 8, 4096)]:
        assert K.describe(B, H, Hkv, N, N, 72, has_nk=True) == V4
        assert K.describe(B, H, Hkv, N, N, 72, has_nk=True, has_text=True, Tkpad=128) == V4
        assert K.describe(B, H, Hkv, N, N, 72, has_nk=False) == V4 == X.describe(B, H, Hkv, N, N, 72)
        # 320 text keys, ragged layouts and attention_variant 3 keep the ping-pong kernel
        assert K.describe(B, H, Hkv, N, N, 72, has_nk=True, has_text=True, Tkpad=320) == "attn_fwd_kernel_v3<72>"
    assert K.describe(2, 4, 4, 200, 200, 72, has_nk=True) == "attn_fwd_kernel_v3<72>"
    # the other head dims have no key count in their one-wave kernels: today's kernels
    set_option("attention_variant", 6)
    assert K.describe(2, 32, 32, 4096, 4096, 48, has_nk=True) == "attn_fwd_kernel_v2<48>" and K.describe(2, 32, 32, 4096, 4096, 48, has_nk=False) == "attn_fwd_kernel_v4h48"
    set_option("attention_variant", 4)
    assert K.describe(2, 4, 4, 320, 320, 96, has_nk=True) == "attn_fwd_kernel_v3<96>" and K.describe(2, 4, 4, 320, 320, 96, has_nk=False) == "attn_fwd_kernel_v4h96"
    assert K.describe(2, 4, 4, 320, 320, 128, has_nk=True) == "attn_fwd_kernel<128>" and K.describe(2, 4, 4, 320, 320, 128, has_nk=False) == "attn_fwd_kernel_hd128"
    set_option("attention_variant", 3)
    assert K.describe(3, 2, 2, 320, 320, 72, has_nk=True) == "attn_fwd_kernel_v3<72>"


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("case", K.SELF_CASES, ids=lambda c: "x".join(map(str, c[:4])) + "-" + "_".join(map(str, c[4])))
def test_key_counts_are_word_exact(case, family):
    B, H, Hkv, N, counts = case
    assert K.describe(B, H, Hkv, N, N, K.HD) == V4
    inp, kp, vp, want = _self(family, case)
    what = f"{V4} nk {family} {case}"
    got = K.run_nk(inp["q"], kp, vp, counts, what=what)
    share = X.assert_attention_words(got, [want], what=what, inp=inp)
    print(f"EXACT-NK family={family} case={case} ambiguous={share:.4%} stats={inp['stats']}")
    if all(n == N for n in counts):  # nk given, nothing masked: the words of the nk_dev = NULL launch
        assert torch.equal(got, K.run_nk(inp["q"], kp, vp, None, what=what + " (NULL)"))


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("case", K.FUSED_CASES, ids=lambda c: f"T{c[5]}-valid{'_'.join(map(str, c[6]))}")
def test_fused_text_phase_behind_a_masked_image_phase(case, skip, family):
    """a stale -inf pad chunk of the last image tile would mask a text key here: slot (5 - 1) & 3 = 0 serves text tile 0"""
    B, H, Hkv, N, counts, T, tvalid = case
    set_option("attn_text_skip", skip)
    assert K.describe(B, H, Hkv, N, N, K.HD, has_text=True, Tkpad=X.pad64(T)) == V4
    a, t = K.fused_draw(family, B, H, Hkv, N, counts, T, tvalid, device="cuda")
    want_self, want_txt = X.expected(a), X.expected(t)
    kp, vp = K.poison_masked(a)
    gate = X.gate_values(H, T, "cuda")
    what = f"{V4} nk + text {family} {case} text_skip {skip}"
    got = K.run_nk(a["q"], kp, vp, counts, what=what, txt=t, gate=gate)
    share = X.assert_attention_words(got, [want_self, want_txt], X.fused(gate), what=what)
    print(f"EXACT-NK fused family={family} case={case} skip={skip} ambiguous={share:.4%}")


@pytest.mark.parametrize("family", K.FAMILIES)
def test_pair_layout_output_holds_the_same_words(family):
    case = (2, 8, 2, 320, (191, 64))  # H * hd = 576: whole 32-column groups, as lt_op_pair_layout asks
    assert case in K.SELF_CASES
    inp, kp, vp, want = _self(family, case)
    plain = K.run_nk(inp["q"], kp, vp, case[4], what="out_pair 0")
    paired = K.run_nk(inp["q"], kp, vp, case[4], out_pair=1, what="out_pair 1")
    assert torch.equal(plain, paired)
    X.assert_attention_words(paired, [want], what=f"out_pair 1 {family}", inp=inp)


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_identical_to_the_ping_pong_kernel_on_random_operands(shape):
    B, H, Hkv = shape
    for N, lists in ((320, K.COUNTS_320), (128, K.COUNTS_128)):
        q, k, v, txt = K.random_operands(B, H, Hkv, N, 128, seed=N + B)
        gate = (torch.randn(H, device="cuda") * 0.5).to(torch.bfloat16)
        for c in lists:
            counts = K.counts_for(B, c)
            out = {}
            for variant in (4, 3):
                set_option("attention_variant", variant)
                assert K.describe(B, H, Hkv, N, N, K.HD, has_text=True, Tkpad=128) == (V4 if variant == 4 else "attn_fwd_kernel_v3<72>")
                out[variant] = (K.run_nk(q, k, v, counts, what=f"variant {variant}"), K.run_nk(q, k, v, counts, what=f"variant {variant} + text", txt=txt, gate=gate))
            set_option("attention_variant", 4)
            for a, b, what in zip(out[4], out[3], ("self", "self + text")):
                assert bool(torch.isfinite(a.float()).all())
                assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), (shape, N, counts, what, int((a != b).sum()))


def test_refusals_name_the_cause_and_leave_the_output_untouched():
    B, H, Hkv, N, hd = 2, 8, 2, 128, 72
    L = lib()
    q = torch.zeros(B, H, N, hd, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(B, Hkv, N, hd, dtype=torch.bfloat16, device="cuda")
    vt = torch.zeros(B, Hkv, hd, N, dtype=torch.bfloat16, device="cuda")
    tb = torch.zeros(B, 64, device="cuda")
    gate = torch.zeros(H, dtype=torch.bfloat16, device="cuda")
    nk = torch.tensor([N, 5], dtype=torch.int32, device="cuda")
    guard = Guarded(B * N, H * hd)
    o = P(guard.out)

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        guard.assert_intact(msg)
        assert bool(torch.isnan(guard.out).all()), msg

    s = stream()
    for args in ((None, P(k), P(vt), o), (P(q), None, P(vt), o), (P(q), P(k), None, o), (P(q), P(k), P(vt), None)):
        qq, kk, vv, oo = args
        refused(L.lt_op_attention_nk(qq, kk, vv, None, oo, None, 0, B, H, Hkv, N, N, N, hd, 1.0, 1, P(nk), 0, s), "lt_op_attention_nk: null")
        refused(L.lt_op_attention_fused_nk(qq, kk, vv, P(k), P(vt), P(tb), P(gate), oo, B, H, Hkv, N, N, N, 64, 64, hd, P(nk), 0, s), "lt_op_attention_fused_nk: null")
    refused(L.lt_op_attention_fused_nk(P(q), P(k), P(vt), None, P(vt), P(tb), P(gate), o, B, H, Hkv, N, N, N, 64, 64, hd, P(nk), 0, s), "lt_op_attention_fused_nk: null")
    refused(L.lt_op_attention_nk_describe(0, 0, B, H, Hkv, N, N, N, hd, 1, 0, 0, None, 64), "lt_op_attention_nk_describe: null")
    # a ragged layout with key counts; bad sizes
    refused(L.lt_op_attention_nk(P(q), P(k), P(vt), None, o, None, 0, B, H, Hkv, N, 100, 128, hd, 1.0, 1, P(nk), 0, s), "lt_op_attention_nk", "Nk % 64")
    refused(L.lt_op_attention_fused_nk(P(q), P(k), P(vt), P(k), P(vt), P(tb), P(gate), o, B, H, Hkv, N, 100, 128, 64, 64, hd, P(nk), 0, s), "lt_op_attention_fused_nk", "Nk % 64")
    refused(L.lt_op_attention_nk(P(q), P(k), P(vt), None, o, None, 0, B, H, Hkv, 0, N, N, hd, 1.0, 1, P(nk), 0, s), "lt_op_attention_nk: bad shape")
    refused(L.lt_op_attention_nk(P(q), P(k), P(vt), None, o, None, 0, B, H, Hkv, N, N, 64, hd, 1.0, 1, P(nk), 0, s), "lt_op_attention_nk: bad shape")
    # the pair layout is written by the one-wave kernels only
    set_option("attention_variant", 3)
    refused(L.lt_op_attention_nk(P(q), P(k), P(vt), None, o, None, 0, B, H, Hkv, N, N, N, hd, 1.0, 1, P(nk), 1, s), "out_pair")
    set_option("attention_variant", 4)
    # q_raw (q_norm + RoPE in the prologue) together with key counts: one rope_grid_w per launch
    f32 = torch.zeros(2 * 384 * 18 * 2, device="cuda")
    refused(L.lt_op_attention_qraw_nk(P(q), 3 * H * hd, 0, P(f32), P(gate), P(gate), P(f32), P(f32), 384, 16, None, 0.0, P(k), P(vt), None, None, None, None, 0, 0, o,
                                      B, H, Hkv, N, N, hd, P(nk), s), "q_raw", "nk_batch")
    refused(L.lt_op_attention_qraw_nk(None, 0, 0, None, None, None, None, None, 0, 0, None, 0.0, None, None, None, None, None, None, 0, 0, None, 1, 1, 1, 64, 64, 72,
                                      None, None), "lt_op_attention_qraw_nk: null")
