"""-m gpu: every attention kernel behind launch_attention on operands whose softmax is exact (tests/exact_attention.py): each output word
must be the one correctly rounded word of the float64 softmax (either neighbour only within DELTA = 2^-20 of a bf16 midpoint), on a
NaN-filled output between sentinel guards.  Every case names the kernel it means to run and asserts it through
lt_op_attention_describe, so a dispatch change cannot move a case to another kernel unnoticed.  (lt_op_attention_describe has no text
arguments: for the fused launches it is asked about the self-attention part, and the cases keep to the text lengths - Tkpad <= 256 on
the one-wave kernels - for which launch_attention's choice is the same; T = 300 runs under attention_variant 3 only.)"""
import pytest

import exact_attention as X
from gpu_util import set_option

pytestmark = pytest.mark.gpu

FAMILIES = ["selector", "levels"]
V1 = "attn_fwd_kernel<%d>"
RAGGED = [(2, 4, 1, 200), (1, 4, 4, 40), (1, 4, 4, 64), (1, 2, 2, 321), (1, 1, 1, 1000)]
UNROLL = [(1, 4, 4, 128), (1, 4, 1, 192), (2, 4, 4, 320), (1, 1, 1, 384), (1, 4, 1, 448)]     # tile counts 2, 3, 5, 6, 7: every remainder of the unrolled loop
LONG = [(1, 4, 4, 64), (2, 4, 1, 256), (1, 2, 2, 1024), (2, 4, 4, 4096)]

# (kernel, attention_variant, head_dim, [(B, H, Hkv, N)])
SELF_CASES = [
    (V1 % 48, 1, 48, RAGGED + UNROLL[:2]),
    (V1 % 72, 1, 72, RAGGED + UNROLL + [(1, 2, 2, 1024)]),
    (V1 % 96, 1, 96, RAGGED + UNROLL[1:3]),
    (V1 % 128, 1, 128, RAGGED + UNROLL[2:4] + [(1, 2, 1, 1024)]),
    (V1 % 128, 4, 128, [(1, 4, 4, 40), (2, 4, 1, 200)]),                      # ragged key counts under the default variant
    ("attn_fwd_kernel_v2<48>", 2, 48, RAGGED + UNROLL + [(1, 2, 2, 1024)]),
    ("attn_fwd_kernel_v2<48>", 4, 48, [(2, 4, 1, 256)]),                       # below ~200 workgroups the default keeps the round-1 kernel
    ("attn_fwd_kernel_v2<72>", 2, 72, RAGGED + UNROLL + [(1, 2, 2, 1024)]),
    ("attn_fwd_kernel_v3<72>", 3, 72, RAGGED + UNROLL + LONG),
    ("attn_fwd_kernel_v3<72>", 4, 72, [(1, 2, 2, 321), (1, 1, 1, 1000)]),
    ("attn_fwd_kernel_v3<96>", 3, 96, RAGGED + UNROLL + LONG[:3] + [(1, 2, 1, 4160)]),
    ("attn_fwd_kernel_v3<96>", 4, 96, [(1, 2, 2, 321), (1, 1, 1, 200)]),
    ("attn_fwd_kernel_v4<72>", 4, 72, UNROLL + LONG + [(1, 2, 2, 4160), (1, 2, 1, 12800)]),
    ("attn_fwd_kernel_v4h48", 6, 48, UNROLL + LONG),
    ("attn_fwd_kernel_v4h96", 4, 96, UNROLL + LONG + [(1, 4, 1, 4160)]),
    ("attn_fwd_kernel_hd128", 4, 128, UNROLL + LONG),
]
SELF_PARAMS = [pytest.param(kern, var, hd, *shape, id=f"{kern}-v{var}-{'x'.join(map(str, shape))}")
               for kern, var, hd, shapes in SELF_CASES for shape in shapes]
# the selector family with the scale applied by the kernel (k_prescaled = 0): one ragged / whole-tile shape per kernel
RAW_PARAMS = [pytest.param(kern, var, hd, *shapes[0], id=f"{kern}-v{var}") for kern, var, hd, shapes in SELF_CASES]


@pytest.fixture(autouse=True)
def _default_options():
    yield
    set_option("attention_variant", 4)
    set_option("attn_text_skip", 1)
    set_option("attn_tail_split", 4)


def _report(kernel, family, shape, share, inp):
    st = inp.get("stats", {})
    print(f"EXACT kernel={kernel} family={family} shape={shape} ambiguous={share:.4%} delta=2^-20 live={st.get('min_live')}..{st.get('max_live')} "
          f"jump_rows={st.get('jump')} small_raise_rows={st.get('small_raise')}")


def _self_case(family, kernel, variant, hd, B, H, Hkv, N, k_prescaled=1):
    try:
        set_option("attention_variant", variant)
        assert X.describe(B, H, Hkv, N, N, hd) == kernel
        inp = X.GENERATORS[family](B, H, Hkv, N, N, hd, seed=N + hd + variant, device="cuda")
        scale = 1.0 if k_prescaled else hd ** -0.5
        want = X.expected(inp, k_prescaled, scale)
        if family == "levels":
            assert X.every_reduction_index_is_used(inp)
            if N > 64:
                assert inp["stats"]["jump"] > 0 and inp["stats"]["small_raise"] > 0, inp["stats"]
        what = f"{kernel} {family} {(B, H, Hkv, N, hd)} k_prescaled {k_prescaled}"
        got = X.run_attention(inp, k_prescaled=k_prescaled, scale=scale, what=what)
        share = X.assert_attention_words(got, [want], what=what, inp=inp)
        _report(kernel, family, (B, H, Hkv, N, hd), share, inp)
    finally:
        set_option("attention_variant", 4)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kernel,variant,hd,B,H,Hkv,N", SELF_PARAMS)
def test_self_attention_is_word_exact(kernel, variant, hd, B, H, Hkv, N, family):
    _self_case(family, kernel, variant, hd, B, H, Hkv, N)


@pytest.mark.parametrize("kernel,variant,hd,B,H,Hkv,N", RAW_PARAMS)
def test_selector_with_the_scale_applied_by_the_kernel(kernel, variant, hd, B, H, Hkv, N):
    """k_prescaled = 0, scale 1 / sqrt(hd): the selected key stays 256 raw units (>= 32 in log2 units) above every other"""
    _self_case("selector", kernel, variant, hd, B, H, Hkv, N, k_prescaled=0)


# lt_op_attention with a key bias and the gated accumulate: (kernel, variant, hd)
BIAS_KERNELS = [(V1 % 72, 1, 72), ("attn_fwd_kernel_v2<72>", 2, 72), ("attn_fwd_kernel_v2<72>", 4, 72), (V1 % 96, 4, 96), ("attn_fwd_kernel_v2<48>", 4, 48),
                (V1 % 128, 4, 128)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T,valid1", [(13, 5), (16, 8), (77, 77), (128, 8), (200, 130)])
@pytest.mark.parametrize("kernel,variant,hd", BIAS_KERNELS)
def test_text_attention_with_bias_and_accumulate_is_word_exact(kernel, variant, hd, T, valid1, family):
    """out = R(prev + R(softmax(q k^T + bias) v * bf16(tanh(gate[h])))): gates from {+20, -20, 0}, prev small integers, a short valid length
    on the second sample; both admissible neighbours of an ambiguous softmax word are carried through the two later roundings"""
    B, H, Hkv, N = 2, 6, 2, 96
    try:
        set_option("attention_variant", variant)
        assert X.describe(B, H, Hkv, N, T, hd, bias=True, accumulate=True) == kernel
        inp = X.GENERATORS[family](B, H, Hkv, N, T, hd, seed=T + hd, valid=(T, valid1), device="cuda")
        want = X.expected(inp)
        gate, prev = X.gate_values(H, T, "cuda"), X.small_int_prev(B, H, N, hd, T, "cuda")
        what = f"{kernel} {family} bias + accumulate T {T} valid {(T, valid1)}"
        got = X.run_attention(inp, use_bias=True, gate=gate, prev=prev, what=what)
        share = X.assert_attention_words(got, [want], X.gated(prev, gate), what=what)
        _report(kernel, family, (B, H, Hkv, N, hd, T, valid1), share, inp)
    finally:
        set_option("attention_variant", 4)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,valid1", [(128, 40), (200, 130), (64, 64)])
def test_hd128_with_a_key_bias_is_word_exact(N, valid1, family):
    B, H, Hkv, hd = 2, 4, 2, 128
    assert X.describe(B, H, Hkv, N, N, hd, bias=True) == V1 % 128
    inp = X.GENERATORS[family](B, H, Hkv, N, N, hd, seed=N, valid=(N, valid1), device="cuda")
    want = X.expected(inp)
    what = f"{V1 % 128} {family} key bias {(N, valid1)}"
    got = X.run_attention(inp, use_bias=True, what=what)
    share = X.assert_attention_words(got, [want], what=what, inp=inp)
    _report(V1 % 128, family, (B, H, Hkv, N, hd, valid1), share, inp)


def _fused_case(family, kernel, variant, hd, B, H, Hkv, N, T, valid, skip=1, split=4):
    try:
        set_option("attention_variant", variant)
        set_option("attn_text_skip", skip)
        set_option("attn_tail_split", split)
        assert X.describe(B, H, Hkv, N, N, hd) == kernel
        a, t = X.fused_draw(family, B, H, Hkv, N, T, hd, N + T + hd, valid, "cuda")
        want_self, want_txt = X.expected(a), X.expected(t)
        gate = X.gate_values(H, T, "cuda")
        what = f"{kernel} {family} fused {(B, H, Hkv, N, hd)} T {T} valid {valid} text_skip {skip} tail_split {split}"
        got = X.run_attention_fused(a, t, gate, what=what)
        share = X.assert_attention_words(got, [want_self, want_txt], X.fused(gate), what=what)
        _report(kernel + "+text", family, (B, H, Hkv, N, hd, T, valid, skip, split), share, t)
    finally:
        set_option("attention_variant", 4)
        set_option("attn_text_skip", 1)
        set_option("attn_tail_split", 4)


FUSED_SHAPES = [(2, 6, 2, 320, 128, (128, 8)), (2, 3, 3, 192, 77, (77, 1)), (1, 6, 6, 1024, 256, (256,)), (2, 6, 2, 256, 200, (60, 130)),
                (2, 3, 1, 128, 64, (64, 33))]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,H,Hkv,N,T,valid", FUSED_SHAPES)
@pytest.mark.parametrize("hd,variant,skip", [(72, 3, 1), (72, 4, 0), (72, 4, 1), (96, 3, 1), (96, 4, 0), (96, 4, 1)])
def test_fused_text_attention_is_word_exact(hd, variant, skip, B, H, Hkv, N, T, valid, family):
    """R(R(self) + R(R(text) * gate)) in one launch: the ping-pong kernels (variant 3) and the one-wave kernels with the text-tile skip off
    and on; valid lengths 1, 8 and T among them"""
    kernel = {(72, 3): "attn_fwd_kernel_v3<72>", (72, 4): "attn_fwd_kernel_v4<72>", (96, 3): "attn_fwd_kernel_v3<96>", (96, 4): "attn_fwd_kernel_v4h96"}[hd, variant]
    _fused_case(family, kernel, variant, hd, B, H, Hkv, N, T, valid, skip=skip)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("hd", [72, 96])
def test_fused_text_attention_300_text_keys_on_the_ping_pong_kernel(hd, family):
    _fused_case(family, f"attn_fwd_kernel_v3<{hd}>", 3, hd, 2, 6, 6, 128, 300, (300, 130))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("parts", [0, 2, 3, 4])
@pytest.mark.parametrize("B,H,Hkv,N,T,valid", [(1, 4, 1, 2112, 0, ()), (1, 2, 2, 2176, 0, ()), (1, 3, 3, 2112, 128, (77,))])
def test_hd96_tail_split_is_word_exact(B, H, Hkv, N, T, valid, parts, family):
    """the partial last query block (N % 256 = 64 or 128 rows) as `parts` workgroups over disjoint key ranges + the merge launch: the merged
    rows are held to the same criterion as every other row; row classes put the maximum of tail rows into the last tiles as well"""
    hd, kernel = 96, "attn_fwd_kernel_v4h96"
    assert N % 256 in (64, 128) and N // 64 >= 8 * max(parts, 1)
    if T:
        return _fused_case(family, kernel, 4, hd, B, H, Hkv, N, T, valid, split=parts)
    try:
        set_option("attn_tail_split", parts)
        assert X.describe(B, H, Hkv, N, N, hd) == kernel
        inp = X.GENERATORS[family](B, H, Hkv, N, N, hd, seed=N + parts, device="cuda")
        want = X.expected(inp)
        what = f"{kernel} {family} {(B, H, Hkv, N, hd)} tail_split {parts}"
        got = X.run_attention(inp, what=what)
        share = X.assert_attention_words(got, [want], what=what, inp=inp)
        _report(kernel + (f"+merge{parts}" if parts else ""), family, (B, H, Hkv, N, hd), share, inp)
    finally:
        set_option("attn_tail_split", 4)
