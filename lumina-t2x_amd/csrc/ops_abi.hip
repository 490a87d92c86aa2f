// Operator-level entry points of the C ABI (lt_op_*, include/lumina_dit_debug.h): each one fills the argument struct of ONE launcher (or of
// the two launches the engine makes back to back) from plain arguments, for the parity tests and the operator benchmarks.  None of them
// touches an engine object; they see the process-default options (lt_set_option).
#include <cstdio>
#include <cstring>

#include "../../include/lumina_dit.h"
#include "../../include/lumina_dit_debug.h"
#include "common.h"
#include "kernels.h"
#include "options.h"

extern "C" int lt_op_gemm_bf16(const void* A, const void* W, const void* bias, int32_t bias_dtype, void* C, int32_t M,
                               int32_t N, int32_t K, int32_t epilogue, int32_t variant, void* stream) {
    LT_REQUIRE(A && W && C, "lt_op_gemm_bf16: null pointer");
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = epilogue == 1 ? N / 2 : N; g.bias_dtype = bias ? bias_dtype : -1;
    return launch_gemm_bf16(g, epilogue, variant, (hipStream_t)stream);
}

// round 6: the row-pair-interleaved operand layout of the persistent GEMM (GemmArgs::pair_ab) at the op level
extern "C" int lt_op_pair_layout(void* m, int64_t rows, int32_t cols, int32_t to_pair, void* stream) {
    LT_REQUIRE(m, "lt_op_pair_layout: null pointer");
    return launch_pair_layout((u16*)m, rows, cols, to_pair, (hipStream_t)stream);
}
extern "C" int lt_op_gemm_bf16_pair(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t pair_c,
                                    void* stream) {
    LT_REQUIRE(A && W && C, "lt_op_gemm_bf16_pair: null pointer");
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = nullptr; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = epilogue == 1 ? N / 2 : N; g.bias_dtype = -1; g.pair_ab = 3; g.pair_c = pair_c;
    return launch_gemm_bf16(g, epilogue, 0, (hipStream_t)stream);
}

extern "C" int lt_op_gemm_vt(const void* A, const void* W, void* vt, int32_t M, int32_t N, int32_t K, int32_t tokens, int32_t hd,
                             int32_t variant, void* stream) {
    LT_REQUIRE(A && W && vt, "lt_op_gemm_vt: null pointer");
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)vt; g.bias = nullptr; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = 0; g.bias_dtype = -1; g.vt_tokens = tokens; g.vt_hd = hd; g.vt_npad = tokens;
    return launch_gemm_bf16(g, 2, variant, (hipStream_t)stream);
}

extern "C" int lt_op_gemm_qkv(const void* A, const void* W, void* C, void* vt, int32_t M, int32_t N, int32_t K, int32_t split,
                              int32_t tokens, int32_t hd, void* stream) {
    LT_REQUIRE(A && W && C && vt, "lt_op_gemm_qkv: null pointer");
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = nullptr; g.bias_dtype = -1; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = N; g.VT = (u16*)vt; g.vt_split = split; g.vt_tokens = tokens; g.vt_hd = hd; g.vt_npad = tokens;
    return launch_gemm_bf16(g, 3, 0, (hipStream_t)stream);
}

// The fused QKV launch with the Q columns' LayerNorm partials (GemmArgs::qstat) followed by the K pass of qk_norm_rope that reduces
// them (QkPostArgs::qstat_in): exactly the two launches the engine makes per layer on the attn_q_fused path.
extern "C" int lt_op_qkv_qstat(const void* A, const void* W, void* C, void* vt, int32_t M, int32_t N, int32_t K, int32_t split, int32_t tokens,
                               int32_t hd, int32_t q_cols, const void* k_ln_w, const void* k_ln_b, const void* cs_table, int32_t grid_w,
                               float k_out_scale, void* k_out, void* qstat_ws, void* q_mean_rstd, void* stream) {
    LT_REQUIRE(A && W && C && vt && k_ln_w && k_ln_b && cs_table && k_out && qstat_ws && q_mean_rstd, "lt_op_qkv_qstat: null pointer");
    LT_REQUIRE(hd > 0 && q_cols > 0 && q_cols % hd == 0 && split > q_cols && (split - q_cols) % hd == 0 && M % tokens == 0,
               "lt_op_qkv_qstat: bad column split (q %d | k | v at %d, head_dim %d)", q_cols, split, hd);
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = nullptr; g.bias_dtype = -1; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = N; g.VT = (u16*)vt; g.vt_split = split; g.vt_tokens = tokens; g.vt_hd = hd; g.vt_npad = tokens;
    const int bn = gemm_qkv_tile_width(g);
    LT_REQUIRE(bn > 0 && q_cols % bn == 0 && 2 * q_cols / bn <= 32, "lt_op_qkv_qstat: the problem does not take the fused QKV launch with whole Q tiles");
    g.qstat = (float*)qstat_ws; g.qstat_cols = q_cols; g.qstat_slots = 2 * q_cols / bn;  // qstat_ws: [M][qstat_slots] float2, <= [M][32]
    if (int rc = launch_gemm_bf16(g, 3, 0, (hipStream_t)stream)) return rc;
    QkPostArgs q;
    q.src = (const u16*)C; q.ld_src = N; q.col0 = q_cols; q.ln_w = (const u16*)k_ln_w; q.ln_b = (const u16*)k_ln_b; q.ln_eps = 1e-5f;
    q.dst = (u16*)k_out; q.B = M / tokens; q.N = tokens; q.heads = (split - q_cols) / hd; q.hd = hd; q.rope_mode = 1;
    q.cs = (const float*)cs_table; q.t = nullptr; q.grid_w = grid_w; q.cs_len = 0; q.watershed = 0.f; q.out_scale = k_out_scale;  // (one branch's table, as lt_op_qk_norm_rope)
    q.qstat_in = (const float*)qstat_ws; q.qstat_out = (float*)q_mean_rstd; q.qstat_slots = g.qstat_slots; q.qstat_width = q_cols;
    return launch_qk_norm_rope(q, (hipStream_t)stream);
}

extern "C" int lt_op_gemm_qkv_fusable(int32_t M, int32_t N, int32_t K, int32_t split, int32_t tokens, int32_t hd) {
    GemmArgs g;
    g.A = nullptr; g.W = nullptr; g.C = nullptr; g.bias = nullptr; g.bias_dtype = -1; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = N; g.VT = (u16*)1; g.vt_split = split; g.vt_tokens = tokens; g.vt_hd = hd; g.vt_npad = tokens;
    return lt_opt(OPT_QKV_FUSED_GEMM) && lt_opt(OPT_QKV_VT_EPILOGUE) && gemm_qkv_fusable(g) ? 1 : 0;
}

extern "C" int lt_op_gemm_describe(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t variant, char* out, int32_t cap) {
    LT_REQUIRE(out && cap > 0, "lt_op_gemm_describe: null buffer");
    GemmArgs g;
    g.A = nullptr; g.W = nullptr; g.C = nullptr; g.bias = nullptr; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = epilogue == 1 ? N / 2 : N; g.bias_dtype = -1;
    snprintf(out, (size_t)cap, "%s", lt_gemm_describe(g, epilogue, variant));
    return 0;
}

extern "C" int lt_op_moe_plan(void* sel, const void* sample_logits, void* wts, int32_t rows, int32_t rows_per_sample, int32_t E, void* pos,
                              void* src, void* tile_expert, int32_t max_tiles, void* stream) {
    LT_REQUIRE(sel && pos && src && tile_expert, "lt_op_moe_plan: null pointer");
    LT_REQUIRE(sample_logits == nullptr || wts != nullptr, "lt_op_moe_plan: routing from per-sample logits writes the weights too");
    MoeArgs m;
    m.x = nullptr; m.gate_w = nullptr; m.sample_logits = (const u16*)sample_logits; m.forced = nullptr;
    m.rows = rows; m.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : rows; m.d = 8; m.E = E;
    m.sel = (int*)sel; m.wts = (u16*)wts; m.pos = (int*)pos; m.src = (int*)src; m.tile_expert = (int*)tile_expert; m.max_tiles = max_tiles;
    return launch_moe_plan(m, (hipStream_t)stream);
}

// lt_op_moe_plan with MoeArgs whole: the parity hook's forced table, the row stride of the logits and the all-layers form.  The launcher's own
// refusals apply; what it cannot see - that the layers' slices do not overlap - is checked here
extern "C" int lt_op_moe_plan_ex(void* sel, const void* sample_logits, int32_t sample_ld, const void* forced, void* wts, int32_t rows,
                                 int32_t rows_per_sample, int32_t E, void* pos, void* src, void* tile_expert, int32_t max_tiles, int32_t layers,
                                 int64_t layer_stride_rows, int64_t layer_stride_src, int64_t layer_stride_tiles, void* stream) {
    LT_REQUIRE(sel && pos && src && tile_expert, "lt_op_moe_plan_ex: null pointer");
    LT_REQUIRE(sample_logits == nullptr || wts != nullptr, "lt_op_moe_plan_ex: routing from per-sample logits writes the weights too");
    LT_REQUIRE((sample_ld == 0 && layers <= 1) || (sample_logits && E > 0 && (long long)sample_ld >= (long long)(layers > 1 ? layers : 1) * E),
               "lt_op_moe_plan_ex: sample_ld = %d is shorter than the %d logit columns of a sample", sample_ld, (layers > 1 ? layers : 1) * E);
    LT_REQUIRE(layers >= 1, "lt_op_moe_plan_ex: layers = %d", layers);
    LT_REQUIRE(layers == 1 || (rows > 0 && max_tiles > 0 && layer_stride_rows >= 2LL * rows && layer_stride_rows % 2 == 0 &&
                               layer_stride_src >= 256LL * max_tiles && layer_stride_tiles >= max_tiles),
               "lt_op_moe_plan_ex: the layer strides (%lld, %lld, %lld) are shorter than one layer's plan (even and >= %lld, >= %lld, >= %d)",
               (long long)layer_stride_rows, (long long)layer_stride_src, (long long)layer_stride_tiles, 2LL * rows, 256LL * max_tiles, max_tiles);
    MoeArgs m;
    m.x = nullptr; m.gate_w = nullptr; m.sample_logits = (const u16*)sample_logits; m.sample_ld = sample_ld; m.forced = (const int*)forced;
    m.rows = rows; m.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : rows; m.d = 8; m.E = E;
    m.sel = (int*)sel; m.wts = (u16*)wts; m.pos = (int*)pos; m.src = (int*)src; m.tile_expert = (int*)tile_expert; m.max_tiles = max_tiles;
    m.layers = layers; m.layer_stride_rows = layer_stride_rows; m.layer_stride_src = layer_stride_src; m.layer_stride_tiles = layer_stride_tiles;
    return launch_moe_plan(m, (hipStream_t)stream);
}

extern "C" int lt_op_gemm_splitk(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, void* part_f32, void* counters_u32,
                                 int32_t tiles, void* stream) {
    LT_REQUIRE(A && W && C && part_f32 && counters_u32, "lt_op_gemm_splitk: null pointer");
    LT_REQUIRE(M > 0 && N > 0 && K > 0, "lt_op_gemm_splitk: empty problem");
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = nullptr; g.bias_dtype = -1; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N;
    g.splitk_part = (float*)part_f32; g.splitk_cnt = (unsigned*)counters_u32; g.splitk_tiles = tiles;
    return launch_gemm_bf16(g, 0, 8, (hipStream_t)stream);  // variant 8 = the 64 x 128 tile, the only one that splits
}

// the same workspace with the kernel and the split left to the launcher, as in the engine (variant 0): two ways on 64 x 128 tiles, or - round 5,
// K >= 4096 - four ways on 128 x 128 tiles, or none
extern "C" int lt_op_gemm_splitk_auto(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, void* part_f32, void* counters_u32,
                                      int32_t slots, void* stream) {
    LT_REQUIRE(A && W && C && part_f32 && counters_u32, "lt_op_gemm_splitk_auto: null pointer");
    LT_REQUIRE(M > 0 && N > 0 && K > 0, "lt_op_gemm_splitk_auto: empty problem");
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = nullptr; g.bias_dtype = -1; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N;
    g.splitk_part = (float*)part_f32; g.splitk_cnt = (unsigned*)counters_u32; g.splitk_tiles = slots;
    return launch_gemm_bf16(g, 0, 0, (hipStream_t)stream);
}

extern "C" int lt_op_gemm_grouped(const void* A, const void* W, const void* tile_expert, int64_t w_expert_stride, void* C,
                                  int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t variant, void* stream) {
    LT_REQUIRE(A && W && C && tile_expert, "lt_op_gemm_grouped: null pointer");
    LT_REQUIRE(M > 0 && M % 256 == 0, "lt_op_gemm_grouped: M=%d must be a positive multiple of 256 (expert segments)", M);
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = nullptr; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = epilogue == 1 ? N / 2 : N; g.bias_dtype = -1;
    g.tile_expert = (const int*)tile_expert; g.w_expert_stride = w_expert_stride;
    return launch_gemm_bf16(g, epilogue, variant, (hipStream_t)stream);
}

// lt_op_gemm_grouped on the persistent kernel (variant 15) with the tail split of round 6: the tiles of a partial last round of the walk are cut
// along K into 2 / 4 parts that hand fp32 accumulators through tail_part_f32 ([cap_parts][256 x 256] floats) and count in on counters_u32
// ([number of CUs] words, zero before the first launch; every launch leaves them zero)
extern "C" int lt_op_gemm_grouped_tail(const void* A, const void* W, const void* tile_expert, int64_t w_expert_stride, void* C, int32_t M, int32_t N,
                                       int32_t K, void* tail_part_f32, void* counters_u32, int32_t cap_parts, void* stream) {
    LT_REQUIRE(A && W && C && tile_expert && tail_part_f32 && counters_u32 && cap_parts > 0, "lt_op_gemm_grouped_tail: null pointer");
    LT_REQUIRE(M > 0 && M % 256 == 0, "lt_op_gemm_grouped_tail: M=%d must be a positive multiple of 256 (expert segments)", M);
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = nullptr; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = N; g.bias_dtype = -1;
    g.tile_expert = (const int*)tile_expert; g.w_expert_stride = w_expert_stride;
    g.tail_part = (float*)tail_part_f32; g.tail_cnt = (unsigned*)counters_u32; g.tail_cap_parts = cap_parts;
    return launch_gemm_bf16(g, 0, 15, (hipStream_t)stream);
}

extern "C" int lt_op_gemm_grouped_gather(const void* A, int32_t a_rows, const void* row_map, const void* W, const void* tile_expert,
                                         int64_t w_expert_stride, void* C, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t variant,
                                         void* stream) {
    LT_REQUIRE(A && W && C && tile_expert && row_map, "lt_op_gemm_grouped_gather: null pointer");
    LT_REQUIRE(M > 0 && M % 256 == 0 && a_rows > 0, "lt_op_gemm_grouped_gather: M=%d must be a positive multiple of 256, a_rows > 0", M);
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = nullptr; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = epilogue == 1 ? N / 2 : N; g.bias_dtype = -1;
    g.tile_expert = (const int*)tile_expert; g.w_expert_stride = w_expert_stride;
    g.a_row_map = (const int*)row_map; g.a_map_rows = a_rows;
    return launch_gemm_bf16(g, epilogue, variant, (hipStream_t)stream);
}

extern "C" int lt_op_pack_w13(const void* w1, const void* w3, void* out, int32_t F, int32_t K, void* stream) {
    LT_REQUIRE(w1 && w3 && out, "lt_op_pack_w13: null pointer");
    return launch_pack_w13((const u16*)w1, (const u16*)w3, (u16*)out, F, K, (hipStream_t)stream);
}

extern "C" int lt_op_rmsnorm_mod(const void* x, const void* w, const void* scale, const void* shift, int32_t ld_mod,
                                 void* out, int32_t B, int32_t N, int32_t d, float eps, int32_t scale_pre, void* stream) {
    LT_REQUIRE(x && out, "lt_op_rmsnorm_mod: null pointer");
    NormModArgs n;
    n.x = (const u16*)x; n.w = (const u16*)w; n.scale = (const u16*)scale; n.shift = (const u16*)shift; n.out = (u16*)out;
    n.rows = B * N; n.rows_per_batch = N; n.d = d; n.ld_mod = ld_mod; n.eps = eps; n.scale_pre = scale_pre;
    return launch_rmsnorm_mod(n, (hipStream_t)stream);
}

extern "C" int lt_op_gated_residual_norm(void* x, const void* y, const void* post_w, const void* gate, int32_t post_mode,
                                         int32_t gate_mode, const void* next_w, const void* next_scale,
                                         const void* next_shift, int32_t next_mode, int32_t ld_mod, void* h, int32_t B,
                                         int32_t N, int32_t d, float eps, float eps_next, int32_t scale_pre, void* stream) {
    LT_REQUIRE(x && y, "lt_op_gated_residual_norm: null pointer");
    GatedResArgs g;
    g.x = (u16*)x; g.y = (const u16*)y; g.post_w = (const u16*)post_w; g.gate = (const u16*)gate;
    g.next_w = (const u16*)next_w; g.next_scale = (const u16*)next_scale; g.next_shift = (const u16*)next_shift;
    g.h = (u16*)h; g.rows = B * N; g.rows_per_batch = N; g.d = d; g.ld_mod = ld_mod; g.post_mode = post_mode;
    g.gate_mode = gate_mode; g.next_mode = next_mode; g.eps = eps; g.eps_next = eps_next; g.scale_pre = scale_pre;
    return launch_gated_residual_norm(g, (hipStream_t)stream);
}

// The O / W2 projection followed by the sandwich-norm row step - exactly the two launches the engine makes per branch.  use_ystat 1: the
// GEMM's epilogue leaves the rows' sum-of-squares partials in ystat_ws and the row kernel runs its streaming form on them (option grn_ystat's
// path; refused when the problem does not take the persistent kernel's plain dense tiles); 0: the row kernel reduces y itself.
extern "C" int lt_op_proj_gated_residual_norm(const void* A, const void* W, void* y, void* ystat_ws, int32_t ystat_cap, int32_t K, void* x,
                                              const void* post_w, const void* gate, const void* next_w, const void* next_scale, int32_t ld_mod,
                                              void* h, int32_t B, int32_t N, int32_t d, float eps, int32_t use_ystat, void* stream) {
    LT_REQUIRE(A && W && y && x && post_w && gate && next_w && next_scale && h, "lt_op_proj_gated_residual_norm: null pointer");
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)y; g.bias = nullptr; g.M = B * N; g.N = d; g.K = K; g.lda = K; g.ldw = K; g.ldc = d;
    g.bias_dtype = -1;
    GatedResArgs r;
    if (use_ystat) {
        const int ys = gemm_ystat_slots(g, 0);
        LT_REQUIRE(ys > 0, "lt_op_proj_gated_residual_norm: this problem does not run on the persistent kernel's plain dense tiles (no ystat)");
        LT_REQUIRE(ystat_ws && ystat_cap >= ys, "lt_op_proj_gated_residual_norm: ystat workspace of %d floats per row, the launch fills %d", ystat_cap, ys);
        g.ystat = (float*)ystat_ws; g.ystat_slots = ys;
        r.ystat = (const float*)ystat_ws; r.ystat_slots = ys;
    }
    if (int rc = launch_gemm_bf16(g, 0, 0, (hipStream_t)stream)) return rc;
    r.x = (u16*)x; r.y = (const u16*)y; r.post_w = (const u16*)post_w; r.gate = (const u16*)gate; r.next_w = (const u16*)next_w;
    r.next_scale = (const u16*)next_scale; r.next_shift = nullptr; r.h = (u16*)h; r.rows = B * N; r.rows_per_batch = N; r.d = d; r.ld_mod = ld_mod;
    r.post_mode = 1; r.gate_mode = 0; r.next_mode = 1; r.eps = eps; r.eps_next = 1e-6f; r.scale_pre = 1;
    return launch_gated_residual_norm(r, (hipStream_t)stream);
}

// The projection of lt_op_proj_gated_residual_norm ALONE, as the engine's gemm() launches O and W2 at large M: the plain dense GEMM, variant 0,
// with GemmArgs::ystat.  Every closing step the families have (shift, next_mode 2, Flag-DiT's gate form) can then follow through
// lt_op_gated_residual_norm_ex; tests/forward_chain.py
extern "C" int lt_op_gemm_ystat(const void* A, const void* W, void* C, void* ystat_ws, int32_t ystat_cap, int32_t M, int32_t N, int32_t K,
                                int32_t* slots_out, void* stream) {
    LT_REQUIRE(A && W && C && ystat_ws && slots_out, "lt_op_gemm_ystat: null pointer");
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)C; g.bias = nullptr; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N;
    g.bias_dtype = -1;
    const int ys = gemm_ystat_slots(g, 0);
    LT_REQUIRE(ys > 0, "lt_op_gemm_ystat: this problem does not run on the persistent kernel's plain dense tiles (no ystat)");
    LT_REQUIRE(ystat_cap >= ys, "lt_op_gemm_ystat: ystat workspace of %d floats per row, the launch fills %d", ystat_cap, ys);
    g.ystat = (float*)ystat_ws; g.ystat_slots = ys;
    *slots_out = ys;
    return launch_gemm_bf16(g, 0, 0, (hipStream_t)stream);
}

extern "C" int lt_op_prep_mod(void* mod, int32_t B, int32_t ld_mod, int32_t L, int32_t chunks, int32_t d, uint32_t tanh_mask,
                              uint32_t scale_mask, int32_t final_scale_chunk, void* stream) {
    LT_REQUIRE(mod, "lt_op_prep_mod: null pointer");
    return launch_prep_mod((u16*)mod, B, ld_mod, L, chunks, d, tanh_mask, scale_mask, final_scale_chunk, (hipStream_t)stream);
}

extern "C" int lt_op_qk_norm_rope(const void* src, int32_t ld_src, int32_t col0, const void* ln_w, const void* ln_b,
                                  float ln_eps, void* dst, int32_t B, int32_t N, int32_t heads, int32_t hd,
                                  int32_t rope_mode, const void* cs_table, int32_t grid_w, float out_scale, void* stream) {
    LT_REQUIRE(src && dst, "lt_op_qk_norm_rope: null pointer");
    QkPostArgs q;
    q.src = (const u16*)src; q.ld_src = ld_src; q.col0 = col0; q.ln_w = (const u16*)ln_w; q.ln_b = (const u16*)ln_b;
    q.ln_eps = ln_eps; q.dst = (u16*)dst; q.B = B; q.N = N; q.heads = heads; q.hd = hd; q.rope_mode = rope_mode;
    q.cs = (const float*)cs_table; q.t = nullptr; q.grid_w = grid_w > 0 ? grid_w : 1; q.watershed = 0.f;
    q.out_scale = out_scale;
    q.cs_len = 0;  // op level: the caller hands over the single branch table it wants (no branch offset)
    return launch_qk_norm_rope(q, (hipStream_t)stream);
}

// ---- the row kernels with every argument of their launchers exposed (include/lumina_dit_debug.h; tests/test_gpu_rows_exact.py) ---------
extern "C" int lt_op_rmsnorm_mod_ex(const void* x, const void* w, const void* scale, const void* shift, int32_t ld_mod, void* out, int32_t B,
                                    int32_t N, int32_t d, float eps, int32_t scale_pre, int32_t out_pair, void* stream) {
    LT_REQUIRE(x && out, "lt_op_rmsnorm_mod_ex: null pointer");
    NormModArgs n;
    n.x = (const u16*)x; n.w = (const u16*)w; n.scale = (const u16*)scale; n.shift = (const u16*)shift; n.out = (u16*)out;
    n.rows = B * N; n.rows_per_batch = N; n.d = d; n.ld_mod = ld_mod; n.eps = eps; n.scale_pre = scale_pre; n.out_pair = out_pair;
    return launch_rmsnorm_mod(n, (hipStream_t)stream);
}

static void fill_gated_res(GatedResArgs& g, void* x, const void* y, const void* post_w, const void* gate, int post_mode, int gate_mode,
                           const void* next_w, const void* next_scale, const void* next_shift, int next_mode, int ld_mod, void* h, int B, int N,
                           int d, float eps, float eps_next, int scale_pre, int h_pair, const void* ystat, int ystat_slots, const void* moe_ys,
                           const void* moe_pos, const void* moe_wts, const void* route_w, int route_E, void* route_sel, void* route_wts,
                           const void* route_forced) {
    g.x = (u16*)x; g.y = (const u16*)y; g.post_w = (const u16*)post_w; g.gate = (const u16*)gate;
    g.next_w = (const u16*)next_w; g.next_scale = (const u16*)next_scale; g.next_shift = (const u16*)next_shift;
    g.h = (u16*)h; g.rows = B * N; g.rows_per_batch = N; g.d = d; g.ld_mod = ld_mod; g.post_mode = post_mode;
    g.gate_mode = gate_mode; g.next_mode = next_mode; g.eps = eps; g.eps_next = eps_next; g.scale_pre = scale_pre; g.h_pair = h_pair;
    g.ystat = (const float*)ystat; g.ystat_slots = ystat_slots;
    g.moe_ys = (const u16*)moe_ys; g.moe_pos = (const int*)moe_pos; g.moe_wts = (const u16*)moe_wts;
    g.route_w = (const u16*)route_w; g.route_E = route_E; g.route_sel = (int*)route_sel; g.route_wts = (u16*)route_wts;
    g.route_forced = (const int*)route_forced;
}

// ystat: [B * N][ystat_slots] floats, the partial sums of squares of y's rows as a plain input (the streaming kernel without a GEMM in front);
// moe_*: the combine-on-load; route_*: routing on the way out (GatedResArgs)
extern "C" int lt_op_gated_residual_norm_ex(void* x, const void* y, const void* post_w, const void* gate, int32_t post_mode, int32_t gate_mode,
                                            const void* next_w, const void* next_scale, const void* next_shift, int32_t next_mode, int32_t ld_mod,
                                            void* h, int32_t B, int32_t N, int32_t d, float eps, float eps_next, int32_t scale_pre, int32_t h_pair,
                                            const void* ystat, int32_t ystat_slots, const void* moe_ys, const void* moe_pos, const void* moe_wts,
                                            const void* route_w, int32_t route_E, void* route_sel, void* route_wts, const void* route_forced,
                                            void* stream) {
    LT_REQUIRE(x && (y || moe_pos), "lt_op_gated_residual_norm_ex: null pointer");
    GatedResArgs g;
    fill_gated_res(g, x, y, post_w, gate, post_mode, gate_mode, next_w, next_scale, next_shift, next_mode, ld_mod, h, B, N, d, eps, eps_next, scale_pre,
                   h_pair, ystat, ystat_slots, moe_ys, moe_pos, moe_wts, route_w, route_E, route_sel, route_wts, route_forced);
    return launch_gated_residual_norm(g, (hipStream_t)stream);
}

// has_*: only the nullness of the pointers takes part in the dispatch
extern "C" int lt_op_gated_residual_norm_describe(int32_t post_mode, int32_t gate_mode, int32_t next_mode, int32_t d, int32_t has_next_w,
                                                  int32_t has_next_scale, int32_t has_next_shift, int32_t scale_pre, int32_t has_ystat,
                                                  int32_t ystat_slots, int32_t has_moe, char* out, int32_t cap) {
    LT_REQUIRE(out && cap > 0, "lt_op_gated_residual_norm_describe: null buffer");
    const void* some = out;
    GatedResArgs g;
    fill_gated_res(g, out, has_moe ? nullptr : some, some, some, post_mode, gate_mode, has_next_w ? some : nullptr, has_next_scale ? some : nullptr,
                   has_next_shift ? some : nullptr, next_mode, d, out, 1, 1, d, 1e-5f, 1e-6f, scale_pre, 0, has_ystat ? some : nullptr, ystat_slots,
                   has_moe ? some : nullptr, has_moe ? some : nullptr, has_moe ? some : nullptr, nullptr, 0, nullptr, nullptr, nullptr);
    snprintf(out, (size_t)cap, "%s", gated_residual_norm_describe(g));
    return 0;
}

// launch_qkv_post trusts the engine's arguments; at the op level they get the checks of the single and the pair launcher (qkv_post.hip)
static int validate_qk_post_abi(const QkPostArgs& a, const char* who) {
    const int width = a.heads * a.hd;
    LT_REQUIRE(a.B > 0 && a.N > 0 && a.heads > 0 && a.hd > 0 && a.hd % 8 == 0 && a.hd <= 128 && width <= 4096, "%s: bad shape (%d x %d heads x %d)", who, a.B * a.N, a.heads, a.hd);
    LT_REQUIRE(a.ld_src % 8 == 0 && a.col0 % 8 == 0 && a.col0 >= 0 && a.col0 + width <= a.ld_src, "%s: ld_src / col0 must be multiples of 8 and hold the columns", who);
    LT_REQUIRE(a.rope_mode >= 0 && a.rope_mode <= 2 && (a.rope_mode == 0 || a.cs != nullptr), "%s: rotary table missing", who);
    LT_REQUIRE(a.rope_mode != 1 || (a.hd % 4 == 0 && a.grid_w > 0), "%s: 2-D rope needs hd %% 4 == 0 and grid_w > 0", who);
    LT_REQUIRE((a.ln_w == nullptr) == (a.ln_b == nullptr), "%s: LayerNorm weight and bias must come together", who);
    return 0;
}

static void fill_qk_post(QkPostArgs& q, const void* src, int ld_src, int col0, const void* ln_w, const void* ln_b, float ln_eps, void* dst, int B,
                         int N, int heads, int hd, int rope_mode, const void* cs_table, int cs_len, const void* t, float watershed, int grid_w,
                         const void* n_tok_b, const void* grid_w_b, float out_scale) {
    q.src = (const u16*)src; q.ld_src = ld_src; q.col0 = col0; q.ln_w = (const u16*)ln_w; q.ln_b = (const u16*)ln_b;
    q.ln_eps = ln_eps; q.dst = (u16*)dst; q.B = B; q.N = N; q.heads = heads; q.hd = hd; q.rope_mode = rope_mode;
    q.cs = (const float*)cs_table; q.cs_len = cs_len; q.t = (const float*)t; q.watershed = watershed; q.grid_w = grid_w > 0 ? grid_w : 1;
    q.n_tok_b = (const int*)n_tok_b; q.grid_w_b = (const int*)grid_w_b; q.out_scale = out_scale;
}

// cs_table: [2][cs_len][hd / 4 (rope_mode 1) | hd / 2 (rope_mode 2)] (cos, sin), branch 0 below the watershed; t: device float (branch 1 when null);
// n_tok_b / grid_w_b: device int [B] of a packed batch or null; qstat_in: [B * N][qstat_slots] float2 (sum, sum of squares) -> qstat_out [B * N] float2
extern "C" int lt_op_qk_norm_rope_ex(const void* src, int32_t ld_src, int32_t col0, const void* ln_w, const void* ln_b, float ln_eps, void* dst,
                                     int32_t B, int32_t N, int32_t heads, int32_t hd, int32_t rope_mode, const void* cs_table, int32_t cs_len,
                                     const void* t, float watershed, int32_t grid_w, const void* n_tok_b, const void* grid_w_b, float out_scale,
                                     const void* qstat_in, void* qstat_out, int32_t qstat_slots, int32_t qstat_width, void* stream) {
    LT_REQUIRE(src && dst, "lt_op_qk_norm_rope_ex: null pointer");
    QkPostArgs q;
    fill_qk_post(q, src, ld_src, col0, ln_w, ln_b, ln_eps, dst, B, N, heads, hd, rope_mode, cs_table, cs_len, t, watershed, grid_w, n_tok_b, grid_w_b,
                 out_scale);
    q.qstat_in = (const float*)qstat_in; q.qstat_out = (float*)qstat_out; q.qstat_slots = qstat_slots; q.qstat_width = qstat_width;
    return launch_qk_norm_rope(q, (hipStream_t)stream);
}

// q and k of one projection output qkv [B * N, ld] (q at q_col0: heads x hd, k at k_col0: kv_heads x hd) in one persistent launch, as the engine
// calls it at >= 2048 rows
extern "C" int lt_op_qk_norm_rope_pair(const void* qkv, int32_t ld, int32_t q_col0, int32_t k_col0, const void* q_ln_w, const void* q_ln_b,
                                       const void* k_ln_w, const void* k_ln_b, float ln_eps, void* q_dst, void* k_dst, int32_t B, int32_t N,
                                       int32_t heads, int32_t kv_heads, int32_t hd, int32_t rope_mode, const void* cs_table, int32_t cs_len,
                                       const void* t, float watershed, int32_t grid_w, const void* n_tok_b, const void* grid_w_b, float q_out_scale,
                                       float k_out_scale, void* stream) {
    LT_REQUIRE(qkv && q_dst && k_dst, "lt_op_qk_norm_rope_pair: null pointer");
    QkPostArgs q, k;
    fill_qk_post(q, qkv, ld, q_col0, q_ln_w, q_ln_b, ln_eps, q_dst, B, N, heads, hd, rope_mode, cs_table, cs_len, t, watershed, grid_w, n_tok_b, grid_w_b,
                 q_out_scale);
    fill_qk_post(k, qkv, ld, k_col0, k_ln_w, k_ln_b, ln_eps, k_dst, B, N, kv_heads, hd, rope_mode, cs_table, cs_len, t, watershed, grid_w, n_tok_b,
                 grid_w_b, k_out_scale);
    return launch_qk_norm_rope_pair(q, k, (hipStream_t)stream);
}

// the same plus the V transpose (v at v_col0 -> vt_dst [B, kv_heads, hd, Npad]) in ONE launch, as the engine calls it below 2048 rows
extern "C" int lt_op_qkv_post(const void* qkv, int32_t ld, int32_t q_col0, int32_t k_col0, int32_t v_col0, const void* q_ln_w, const void* q_ln_b,
                              const void* k_ln_w, const void* k_ln_b, float ln_eps, void* q_dst, void* k_dst, void* vt_dst, int32_t B, int32_t N,
                              int32_t Npad, int32_t heads, int32_t kv_heads, int32_t hd, int32_t rope_mode, const void* cs_table, int32_t cs_len,
                              const void* t, float watershed, int32_t grid_w, const void* n_tok_b, const void* grid_w_b, float q_out_scale,
                              float k_out_scale, void* stream) {
    LT_REQUIRE(qkv && q_dst && k_dst && vt_dst, "lt_op_qkv_post: null pointer");
    QkvPostArgs a;
    fill_qk_post(a.q, qkv, ld, q_col0, q_ln_w, q_ln_b, ln_eps, q_dst, B, N, heads, hd, rope_mode, cs_table, cs_len, t, watershed, grid_w, n_tok_b,
                 grid_w_b, q_out_scale);
    fill_qk_post(a.k, qkv, ld, k_col0, k_ln_w, k_ln_b, ln_eps, k_dst, B, N, kv_heads, hd, rope_mode, cs_table, cs_len, t, watershed, grid_w, n_tok_b,
                 grid_w_b, k_out_scale);
    if (int rc = validate_qk_post_abi(a.q, "lt_op_qkv_post (q)")) return rc;
    if (int rc = validate_qk_post_abi(a.k, "lt_op_qkv_post (k)")) return rc;
    LT_REQUIRE(ld % 8 == 0 && v_col0 % 8 == 0 && hd % 8 == 0, "lt_op_qkv_post: ld / v_col0 / hd must be multiples of 8");
    a.v_src = (const u16*)qkv; a.v_dst = (u16*)vt_dst; a.v_ld_src = ld; a.v_col0 = v_col0; a.v_B = B; a.v_N = N; a.v_Npad = Npad;
    a.v_kv_heads = kv_heads; a.v_hd = hd;
    return launch_qkv_post(a, (hipStream_t)stream);
}

extern "C" int lt_op_v_transpose(const void* src, int32_t ld_src, int32_t col0, void* dst, int32_t B, int32_t N,
                                 int32_t Npad, int32_t kv_heads, int32_t hd, void* stream) {
    LT_REQUIRE(src && dst, "lt_op_v_transpose: null pointer");
    return launch_v_transpose((const u16*)src, ld_src, col0, (u16*)dst, B, N, Npad, kv_heads, hd, (hipStream_t)stream);
}

extern "C" int lt_op_attention_identity(const void* src, int32_t ld_src, int32_t col0, void* out, int32_t B, int32_t N, int32_t H, int32_t Hkv,
                                        int32_t hd, int32_t out_pair, void* stream) {
    return launch_attention_identity((const u16*)src, ld_src, col0, (u16*)out, B, N, H, Hkv, hd, out_pair, (hipStream_t)stream);
}

extern "C" int lt_op_query_blur(const void* q, void* out, const float* taps_dev, int32_t B, int32_t H, int32_t N, int32_t hd, int32_t grid_w,
                                int32_t blur_w, int32_t radius, int32_t mode, void* stream) {
    return launch_query_blur((const u16*)q, (u16*)out, taps_dev, B, H, N, hd, grid_w, blur_w, radius, mode, (hipStream_t)stream);
}

extern "C" int lt_op_seg_taps(float sigma, float* taps_host, int32_t* radius, int32_t* mode) {
    LT_REQUIRE(taps_host && radius && mode, "lt_op_seg_taps: null argument");
    int r = 0, m = 0;
    if (seg_taps_host(sigma, taps_host, &r, &m)) { lt_set_error("lt_op_seg_taps: sigma %g is not positive", (double)sigma); return 2; }
    *radius = r; *mode = m;
    return 0;
}

extern "C" int lt_op_attention(const void* q, const void* k, const void* vt, const float* bias, void* out, const void* gate,
                               int32_t accumulate, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad,
                               int32_t hd, float scale, int32_t k_prescaled, void* stream) {
    LT_REQUIRE(q && k && vt && out, "lt_op_attention: null pointer");
    AttnArgs a;
    a.q = (const u16*)q; a.k = (const u16*)k; a.vt = (const u16*)vt; a.bias = bias; a.out = (u16*)out;
    a.gate = (const u16*)gate; a.accumulate = accumulate; a.B = B; a.H = H; a.Hkv = Hkv; a.N = N; a.Nk = Nk;
    a.Nkpad = Nkpad; a.hd = hd; a.scale = scale; a.k_prescaled = k_prescaled;
    return launch_attention(a, (hipStream_t)stream);
}

extern "C" int lt_op_attention_describe(int32_t has_bias, int32_t accumulate, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad,
                                        int32_t hd, char* out, int32_t cap) {
    LT_REQUIRE(out && cap > 0, "lt_op_attention_describe: null buffer");
    AttnArgs a;
    a.q = nullptr; a.k = nullptr; a.vt = nullptr; a.bias = has_bias ? (const float*)out : nullptr; a.out = nullptr; a.gate = nullptr;  // (bias: only its nullness is looked at)
    a.accumulate = accumulate; a.B = B; a.H = H; a.Hkv = Hkv; a.N = N; a.Nk = Nk; a.Nkpad = Nkpad; a.hd = hd; a.scale = 1.f;
    snprintf(out, (size_t)cap, "%s", attention_describe(a));
    return 0;
}

// lt_op_attention / lt_op_attention_fused with per-sample image key counts (AttnArgs::nk_batch, the packed batches of the engine) and the
// pair layout of the output (AttnArgs::out_pair): tests/test_gpu_attention_nk.py.  nk NULL: the plain entries' launches.
static int attention_nk_checks(const char* who, const int32_t* nk, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad, int32_t hd) {
    LT_REQUIRE(B > 0 && H > 0 && Hkv > 0 && N > 0 && Nk > 0 && hd > 0 && Nkpad >= Nk, "%s: bad shape B=%d H=%d Hkv=%d N=%d Nk=%d Nkpad=%d hd=%d", who, B, H, Hkv, N,
               Nk, Nkpad, hd);
    LT_REQUIRE(!nk || Nk % 64 == 0, "%s: per-sample key counts need a layout of whole 64-key tiles, Nk %% 64 == 0 (Nk = %d)", who, Nk);
    return 0;
}

extern "C" int lt_op_attention_nk(const void* q, const void* k, const void* vt, const float* bias, void* out, const void* gate, int32_t accumulate,
                                  int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad, int32_t hd, float scale,
                                  int32_t k_prescaled, const int32_t* nk, int32_t out_pair, void* stream) {
    LT_REQUIRE(q && k && vt && out, "lt_op_attention_nk: null pointer");
    if (attention_nk_checks("lt_op_attention_nk", nk, B, H, Hkv, N, Nk, Nkpad, hd)) return 1;
    AttnArgs a;
    a.q = (const u16*)q; a.k = (const u16*)k; a.vt = (const u16*)vt; a.bias = bias; a.out = (u16*)out;
    a.gate = (const u16*)gate; a.accumulate = accumulate; a.B = B; a.H = H; a.Hkv = Hkv; a.N = N; a.Nk = Nk;
    a.Nkpad = Nkpad; a.hd = hd; a.scale = scale; a.k_prescaled = k_prescaled; a.nk_batch = nk; a.out_pair = out_pair;
    return launch_attention(a, (hipStream_t)stream);
}

extern "C" int lt_op_attention_fused_nk(const void* q, const void* k, const void* vt, const void* tk, const void* tvt, const float* tbias,
                                        const void* tgate, void* out, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad,
                                        int32_t Tk, int32_t Tkpad, int32_t hd, const int32_t* nk, int32_t out_pair, void* stream) {
    LT_REQUIRE(q && k && vt && tk && tvt && tbias && tgate && out, "lt_op_attention_fused_nk: null pointer");
    if (attention_nk_checks("lt_op_attention_fused_nk", nk, B, H, Hkv, N, Nk, Nkpad, hd)) return 1;
    LT_REQUIRE(attention_fuses_text(hd), "lt_op_attention_fused_nk: needs head_dim 72 or 96 and attention_variant 3 or 4");
    AttnArgs a;
    a.q = (const u16*)q; a.k = (const u16*)k; a.vt = (const u16*)vt; a.bias = nullptr; a.out = (u16*)out; a.gate = nullptr;
    a.accumulate = 0; a.B = B; a.H = H; a.Hkv = Hkv; a.N = N; a.Nk = Nk; a.Nkpad = Nkpad; a.hd = hd; a.scale = 1.f; a.k_prescaled = 1;
    a.tk = (const u16*)tk; a.tvt = (const u16*)tvt; a.tbias = tbias; a.tgate = (const u16*)tgate; a.Tk = Tk; a.Tkpad = Tkpad;
    a.nk_batch = nk; a.out_pair = out_pair;
    return launch_attention(a, (hipStream_t)stream);
}

// lt_op_attention_describe with the two arguments it lacks: per-sample key counts given, fused text keys given (Tkpad of them)
extern "C" int lt_op_attention_nk_describe(int32_t has_bias, int32_t accumulate, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad,
                                           int32_t hd, int32_t has_nk, int32_t has_text, int32_t Tkpad, char* out, int32_t cap) {
    LT_REQUIRE(out && cap > 0, "lt_op_attention_nk_describe: null buffer");
    LT_REQUIRE(!has_text || (Tkpad > 0 && Tkpad % 64 == 0), "lt_op_attention_nk_describe: has_text needs Tkpad > 0 in whole 64-key tiles (Tkpad = %d)", Tkpad);
    AttnArgs a;
    // (bias, nk_batch, tk: only their nullness is looked at)
    a.q = nullptr; a.k = nullptr; a.vt = nullptr; a.bias = has_bias ? (const float*)out : nullptr; a.out = nullptr; a.gate = nullptr;
    a.accumulate = accumulate; a.B = B; a.H = H; a.Hkv = Hkv; a.N = N; a.Nk = Nk; a.Nkpad = Nkpad; a.hd = hd; a.scale = 1.f;
    a.nk_batch = has_nk ? (const int*)out : nullptr;
    if (has_text) { a.tk = (const u16*)out; a.Tk = Tkpad; a.Tkpad = Tkpad; a.k_prescaled = 1; }
    snprintf(out, (size_t)cap, "%s", attention_describe(a));
    return 0;
}

// self-attention whose queries come straight from the QKV projection (AttnArgs::q_raw): q_norm + 2-D RoPE in the kernel's prologue
extern "C" int lt_op_attention_qraw(const void* qkv, int32_t ld, int32_t q_col0, const void* q_mean_rstd, const void* q_ln_w, const void* q_ln_b,
                                    const void* cs_table, const void* cs_table_t, int32_t table_len, int32_t grid_w, const void* k,
                                    const void* vt, void* out, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nkpad, int32_t hd,
                                    void* stream) {
    LT_REQUIRE(qkv && q_mean_rstd && q_ln_w && q_ln_b && cs_table && cs_table_t && k && vt && out, "lt_op_attention_qraw: null pointer");
    AttnArgs a;
    a.q = nullptr; a.k = (const u16*)k; a.vt = (const u16*)vt; a.bias = nullptr; a.out = (u16*)out; a.gate = nullptr; a.accumulate = 0;
    a.B = B; a.H = H; a.Hkv = Hkv; a.N = N; a.Nk = N; a.Nkpad = Nkpad; a.hd = hd; a.scale = 1.f; a.k_prescaled = 1;
    a.q_raw = (const u16*)qkv; a.q_ld = ld; a.q_col0 = q_col0; a.q_stat = (const float*)q_mean_rstd;
    a.q_ln_w = (const u16*)q_ln_w; a.q_ln_b = (const u16*)q_ln_b;
    a.rope_cs = (const float*)cs_table; a.rope_cs_t = (const float*)cs_table_t; a.rope_t = nullptr; a.rope_watershed = 0.f;  // branch 1
    a.rope_cs_len = table_len; a.rope_grid_w = grid_w;
    return launch_attention(a, (hipStream_t)stream);
}

// lt_op_attention_qraw with the AttnArgs fields the engine fills besides (engine.hip, the attn_q_fused path): the table-branch select (t_dev,
// watershed) and, optionally, the fused text keys (tk == NULL: none).  tests/test_gpu_prologue_exact.py
static int attention_qraw_ex(const char* who, const void* qkv, int32_t ld, int32_t q_col0, const void* q_mean_rstd, const void* q_ln_w, const void* q_ln_b,
                            const void* cs_table, const void* cs_table_t, int32_t table_len, int32_t grid_w, const void* t_dev,
                            float watershed, const void* k, const void* vt, const void* tk, const void* tvt, const float* tbias,
                            const void* tgate, int32_t Tk, int32_t Tkpad, void* out, int32_t B, int32_t H, int32_t Hkv, int32_t N,
                            int32_t Nkpad, int32_t hd, const int32_t* nk, void* stream) {
    LT_REQUIRE(qkv && q_mean_rstd && q_ln_w && q_ln_b && cs_table && cs_table_t && k && vt && out, "%s: null pointer", who);
    AttnArgs a;
    a.nk_batch = nk;
    a.q = nullptr; a.k = (const u16*)k; a.vt = (const u16*)vt; a.bias = nullptr; a.out = (u16*)out; a.gate = nullptr; a.accumulate = 0;
    a.B = B; a.H = H; a.Hkv = Hkv; a.N = N; a.Nk = N; a.Nkpad = Nkpad; a.hd = hd; a.scale = 1.f; a.k_prescaled = 1;
    if (tk) { a.tk = (const u16*)tk; a.tvt = (const u16*)tvt; a.tbias = tbias; a.tgate = (const u16*)tgate; a.Tk = Tk; a.Tkpad = Tkpad; }
    a.q_raw = (const u16*)qkv; a.q_ld = ld; a.q_col0 = q_col0; a.q_stat = (const float*)q_mean_rstd;
    a.q_ln_w = (const u16*)q_ln_w; a.q_ln_b = (const u16*)q_ln_b;
    a.rope_cs = (const float*)cs_table; a.rope_cs_t = (const float*)cs_table_t; a.rope_t = (const float*)t_dev; a.rope_watershed = watershed;
    a.rope_cs_len = table_len; a.rope_grid_w = grid_w;
    return launch_attention(a, (hipStream_t)stream);
}

extern "C" int lt_op_attention_qraw_ex(const void* qkv, int32_t ld, int32_t q_col0, const void* q_mean_rstd, const void* q_ln_w, const void* q_ln_b,
                                       const void* cs_table, const void* cs_table_t, int32_t table_len, int32_t grid_w, const void* t_dev,
                                       float watershed, const void* k, const void* vt, const void* tk, const void* tvt, const float* tbias,
                                       const void* tgate, int32_t Tk, int32_t Tkpad, void* out, int32_t B, int32_t H, int32_t Hkv, int32_t N,
                                       int32_t Nkpad, int32_t hd, void* stream) {
    return attention_qraw_ex("lt_op_attention_qraw_ex", qkv, ld, q_col0, q_mean_rstd, q_ln_w, q_ln_b, cs_table, cs_table_t, table_len, grid_w, t_dev, watershed, k, vt,
                             tk, tvt, tbias, tgate, Tk, Tkpad, out, B, H, Hkv, N, Nkpad, hd, nullptr, stream);
}

// ... plus AttnArgs::nk_batch: the combination launch_attention refuses by name (one rope_grid_w, a packed batch has one per sample); nk NULL:
// lt_op_attention_qraw_ex
extern "C" int lt_op_attention_qraw_nk(const void* qkv, int32_t ld, int32_t q_col0, const void* q_mean_rstd, const void* q_ln_w, const void* q_ln_b,
                                       const void* cs_table, const void* cs_table_t, int32_t table_len, int32_t grid_w, const void* t_dev,
                                       float watershed, const void* k, const void* vt, const void* tk, const void* tvt, const float* tbias,
                                       const void* tgate, int32_t Tk, int32_t Tkpad, void* out, int32_t B, int32_t H, int32_t Hkv, int32_t N,
                                       int32_t Nkpad, int32_t hd, const int32_t* nk, void* stream) {
    return attention_qraw_ex("lt_op_attention_qraw_nk", qkv, ld, q_col0, q_mean_rstd, q_ln_w, q_ln_b, cs_table, cs_table_t, table_len, grid_w, t_dev, watershed, k, vt,
                             tk, tvt, tbias, tgate, Tk, Tkpad, out, B, H, Hkv, N, Nkpad, hd, nk, stream);
}

// launch_attention_small alone (no GEMM in front, no prefetch rider): every field of AttnSmallArgs as a plain argument; ln_eps 1e-5 as in the engine
extern "C" int lt_op_attention_small(const void* qkv, int32_t ld, int32_t q_col0, int32_t k_col0, int32_t v_col0, const void* rowstat, int32_t slots,
                                     int32_t q_slot0, int32_t q_nslot, int32_t k_slot0, int32_t k_nslot, const void* q_ln_w, const void* q_ln_b,
                                     const void* k_ln_w, const void* k_ln_b, const void* cs_table, int32_t table_len, int32_t grid_w,
                                     const void* t_dev, float watershed, float k_scale, void* out, int32_t B, int32_t H, int32_t Hkv,
                                     int32_t tokens, int32_t hd, void* stream) {
    LT_REQUIRE(qkv && rowstat && q_ln_w && q_ln_b && k_ln_w && k_ln_b && cs_table && out, "lt_op_attention_small: null pointer");
    LT_REQUIRE(B > 0 && H > 0 && Hkv > 0 && hd > 0 && tokens > 0, "lt_op_attention_small: bad shape");
    AttnSmallArgs a;
    a.qkv = (const u16*)qkv; a.ld = ld; a.q_col0 = q_col0; a.k_col0 = k_col0; a.v_col0 = v_col0;
    a.rowstat = (const float*)rowstat; a.slots = slots; a.q_slot0 = q_slot0; a.q_nslot = q_nslot; a.k_slot0 = k_slot0; a.k_nslot = k_nslot;
    a.q_ln_w = (const u16*)q_ln_w; a.q_ln_b = (const u16*)q_ln_b; a.k_ln_w = (const u16*)k_ln_w; a.k_ln_b = (const u16*)k_ln_b; a.ln_eps = 1e-5f;
    a.cs = (const float*)cs_table; a.t = (const float*)t_dev; a.watershed = watershed; a.cs_len = table_len; a.grid_w = grid_w;
    a.k_scale = k_scale; a.out = (u16*)out; a.B = B; a.H = H; a.Hkv = Hkv; a.N = tokens; a.hd = hd;
    return launch_attention_small(a, (hipStream_t)stream);
}

// The small-M QKV projection with the per-tile LayerNorm partials (GemmArgs::rowstat) followed by the fused q / k post-processing +
// attention launch (AttnSmallArgs): exactly the two launches the engine makes per layer on the attn_small_fused path.
extern "C" int lt_op_qkv_attention_small(const void* A, const void* W, void* qkv, int32_t M, int32_t K, int32_t H, int32_t Hkv, int32_t tokens,
                                         int32_t hd, const void* q_ln_w, const void* q_ln_b, const void* k_ln_w, const void* k_ln_b,
                                         const void* cs_table, int32_t table_len, int32_t grid_w, float k_scale, void* rowstat_ws,
                                         void* out, void* stream) {
    LT_REQUIRE(A && W && qkv && q_ln_w && q_ln_b && k_ln_w && k_ln_b && cs_table && rowstat_ws && out, "lt_op_qkv_attention_small: null pointer");
    LT_REQUIRE(H > 0 && Hkv > 0 && hd > 0 && tokens > 0 && M > 0 && M % tokens == 0, "lt_op_qkv_attention_small: bad shape");
    const int d = H * hd, dkv = Hkv * hd, N = d + 2 * dkv;
    LT_REQUIRE(attention_small_fusable(hd, tokens, H, Hkv, d, dkv), "lt_op_qkv_attention_small: head_dim 48, 64 <= tokens <= 512 in whole tiles, widths %% 128 == 0");
    GemmArgs g;
    g.A = (const u16*)A; g.W = (const u16*)W; g.C = (u16*)qkv; g.bias = nullptr; g.bias_dtype = -1; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = N;
    LT_REQUIRE(gemm_is_small_m(g, 0), "lt_op_qkv_attention_small: %d x %d x %d does not run on the small-M tiles", M, N, K);
    g.rowstat = (float*)rowstat_ws; g.rowstat_slots = (N + 127) / 128;  // rowstat_ws: [M][ceil(N / 128)] float2
    if (launch_gemm_bf16(g, 0, 0, (hipStream_t)stream)) return 1;
    AttnSmallArgs a;
    a.qkv = (const u16*)qkv; a.ld = N; a.q_col0 = 0; a.k_col0 = d; a.v_col0 = d + dkv;
    a.rowstat = (const float*)rowstat_ws; a.slots = g.rowstat_slots; a.q_slot0 = 0; a.q_nslot = d / 128; a.k_slot0 = d / 128; a.k_nslot = dkv / 128;
    a.q_ln_w = (const u16*)q_ln_w; a.q_ln_b = (const u16*)q_ln_b; a.k_ln_w = (const u16*)k_ln_w; a.k_ln_b = (const u16*)k_ln_b; a.ln_eps = 1e-5f;
    a.cs = (const float*)cs_table; a.t = nullptr; a.watershed = 0.f; a.cs_len = table_len; a.grid_w = grid_w;  // branch 1
    a.k_scale = k_scale; a.out = (u16*)out; a.B = M / tokens; a.H = H; a.Hkv = Hkv; a.N = tokens; a.hd = hd;
    return launch_attention_small(a, (hipStream_t)stream);
}

extern "C" int lt_op_attention_fused(const void* q, const void* k, const void* vt, const void* tk, const void* tvt,
                                     const float* tbias, const void* tgate, void* out, int32_t B, int32_t H, int32_t Hkv, int32_t N,
                                     int32_t Nk, int32_t Nkpad, int32_t Tk, int32_t Tkpad, int32_t hd, void* stream) {
    LT_REQUIRE(q && k && vt && tk && tvt && tbias && tgate && out, "lt_op_attention_fused: null pointer");
    LT_REQUIRE(attention_fuses_text(hd), "lt_op_attention_fused: needs head_dim 72 or 96 and attention_variant 3 or 4");
    AttnArgs a;
    a.q = (const u16*)q; a.k = (const u16*)k; a.vt = (const u16*)vt; a.bias = nullptr; a.out = (u16*)out; a.gate = nullptr;
    a.accumulate = 0; a.B = B; a.H = H; a.Hkv = Hkv; a.N = N; a.Nk = Nk; a.Nkpad = Nkpad; a.hd = hd; a.scale = 1.f; a.k_prescaled = 1;
    a.tk = (const u16*)tk; a.tvt = (const u16*)tvt; a.tbias = tbias; a.tgate = (const u16*)tgate; a.Tk = Tk; a.Tkpad = Tkpad;
    return launch_attention(a, (hipStream_t)stream);
}

extern "C" int lt_op_attention_trace(const void* q, const void* k, const void* vt, void* out, int32_t B, int32_t H, int32_t Hkv,
                                     int32_t N, int32_t Nk, int32_t Nkpad, int32_t hd, float scale, void* trace_dev,
                                     void* stream) {
    LT_REQUIRE(q && k && vt && out && trace_dev, "lt_op_attention_trace: null pointer");
    AttnArgs a;
    a.q = (const u16*)q; a.k = (const u16*)k; a.vt = (const u16*)vt; a.bias = nullptr; a.out = (u16*)out;
    a.gate = nullptr; a.accumulate = 0; a.B = B; a.H = H; a.Hkv = Hkv; a.N = N; a.Nk = Nk;
    a.Nkpad = Nkpad; a.hd = hd; a.scale = scale; a.trace = (unsigned long long*)trace_dev;
    return launch_attention(a, (hipStream_t)stream);
}

extern "C" int lt_op_linear_small_m(const void* a, const void* w, const void* b, void* y, int32_t M, int32_t N, int32_t K,
                                    int32_t act_in, void* stream) {
    LT_REQUIRE(a && w && y, "lt_op_linear_small_m: null pointer");
    return launch_linear_small_m((const u16*)a, (const u16*)w, (const u16*)b, (u16*)y, M, N, K, act_in, (hipStream_t)stream);
}

extern "C" int lt_op_rope_table_2d_pair(void* out, void* out_t, int32_t len, int32_t hd, float theta, float scale_factor, void* stream) {
    LT_REQUIRE(out && out_t, "lt_op_rope_table_2d_pair: null pointer");
    return launch_rope_table_2d((float*)out, len, hd, theta, scale_factor, (hipStream_t)stream, (float*)out_t);
}

extern "C" int lt_op_rope_table_2d(void* out, int32_t len, int32_t hd, float theta, float scale_factor, void* stream) {
    LT_REQUIRE(out, "lt_op_rope_table_2d: null pointer");
    return launch_rope_table_2d((float*)out, len, hd, theta, scale_factor, (hipStream_t)stream);
}

// ---- multi-view sampling (views.hip) and SDE steps (sde.hip) --------------------------------------------------------------------------
extern "C" int lt_op_views_invert(const int32_t* perm_dev, int32_t* iperm_dev, int32_t* hits_dev, int32_t V, int32_t HW, void* stream) {
    return launch_views_invert(perm_dev, iperm_dev, hits_dev, V, HW, (hipStream_t)stream);
}
extern "C" int lt_op_views_gather(const void* y_dev, const int32_t* perm_dev, const float* vsign_dev, const void* f0_dev, void* out_dev, float half_dt,
                                  int32_t V, int32_t C, int32_t HW, int32_t dtype, void* stream) {
    return launch_views_gather(y_dev, perm_dev, vsign_dev, f0_dev, out_dev, half_dt, V, C, HW, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_views_reduce(const void* y_dev, const void* f_dev, const int32_t* iperm_dev, const float* isign_dev, void* out_dev, float dt,
                                  int32_t V, int32_t C, int32_t HW, int32_t dtype, void* stream) {
    return launch_views_reduce(y_dev, f_dev, iperm_dev, isign_dev, out_dev, dt, V, C, HW, dtype, (hipStream_t)stream);
}
// tiled sampling (tiled.hip): the offsets are a HOST table here, checked into a WindowTable before anything is launched
extern "C" int lt_op_windows_gather(const void* y_dev, const int32_t* offsets_host, int32_t n, int32_t win_h, int32_t win_w, int32_t canvas_h,
                                    int32_t canvas_w, void* out_dev, int32_t C, int32_t dtype, void* stream) {
    WindowTable t;
    if (window_table_build("lt_op_windows_gather", offsets_host, n, win_h, win_w, canvas_h, canvas_w, &t)) return 2;
    return launch_windows_gather(y_dev, t, out_dev, C, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_windows_reduce(const void* f_dev, const int32_t* offsets_host, int32_t n, int32_t win_h, int32_t win_w, int32_t canvas_h,
                                    int32_t canvas_w, const float* weight_dev, const float* wsum_dev, void* out_dev, int32_t C, int32_t dtype,
                                    void* stream) {
    WindowTable t;
    if (window_table_build("lt_op_windows_reduce", offsets_host, n, win_h, win_w, canvas_h, canvas_w, &t)) return 2;
    return launch_windows_reduce(f_dev, t, weight_dev, wsum_dev, out_dev, C, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_windows_cover(const int32_t* offsets_host, int32_t n, int32_t win_h, int32_t win_w, int32_t canvas_h, int32_t canvas_w,
                                   const float* weight_dev, float* wsum_dev, int32_t* bad_dev, void* stream) {
    WindowTable t;
    if (window_table_build("lt_op_windows_cover", offsets_host, n, win_h, win_w, canvas_h, canvas_w, &t)) return 2;
    return launch_windows_cover(t, weight_dev, wsum_dev, bad_dev, (hipStream_t)stream);
}
// composed guidance (compose.hip): the weights are a HOST table here; the launchers check everything before anything is launched
extern "C" int lt_op_compose_replicate(const void* y_dev, void* out_dev, int32_t K, int32_t Bp, int32_t C, int32_t HW, int32_t dtype, void* stream) {
    return launch_compose_replicate(y_dev, out_dev, K, Bp, C, HW, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_compose_guidance(const void* f_dev, void* out_dev, const float* w_host, int32_t K, int32_t Bp, int32_t C, int32_t HW,
                                      int32_t cfg_channels, int32_t dtype, void* stream) {
    return launch_compose_guidance(f_dev, out_dev, w_host, K, Bp, C, HW, cfg_channels, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_views_guided_gather(const void* y_dev, const void* guidance_dev, const void* noise_dev, const int32_t* perm_dev,
                                         const float* vsign_dev, const float* isign_dev, const void* f0_dev, void* out_dev, float half_dt,
                                         const float* coef_host, int32_t V, int32_t C, int32_t HW, int32_t dtype, void* stream) {
    return launch_views_guided_gather(y_dev, guidance_dev, noise_dev, perm_dev, vsign_dev, isign_dev, f0_dev, out_dev, half_dt, coef_host, V, C, HW, dtype,
                                      (hipStream_t)stream);
}

extern "C" int lt_op_sde_step(int32_t op, const void* x_dev, const void* v_dev, const void* w_dev, const void* k1_dev, const void* xp_dev,
                              void* out_dev, void* out2_dev, const float* rec_host, int64_t n, int32_t dtype, void* stream) {
    return launch_sde_step(op, x_dev, v_dev, w_dev, k1_dev, xp_dev, out_dev, out2_dev, rec_host, (long long)n, dtype, (hipStream_t)stream);
}

// ---- prompt-driven editing (flowedit.hip) ---------------------------------------------------------------------------------------------
extern "C" int lt_op_flowedit_mix(const void* x_src_dev, const void* z_dev, const void* noise_dev, void* out4_dev, float t, float one_minus_t,
                                  int64_t n_half, int32_t dtype, void* stream) {
    return launch_flowedit_mix(x_src_dev, z_dev, noise_dev, out4_dev, t, one_minus_t, (long long)n_half, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_flowedit_combine(const void* z_dev, const void* out4_dev, void* z_next_dev, float w_s, float w_t, float dt, int32_t Bp, int32_t C,
                                      int32_t HW, int32_t ch, int32_t dtype, void* stream) {
    return launch_flowedit_combine(z_dev, out4_dev, z_next_dev, w_s, w_t, dt, Bp, C, HW, ch, dtype, (hipStream_t)stream);
}

// ---- adaptive Runge-Kutta stepping (ode_adaptive.hip) ---------------------------------------------------------------------------------
extern "C" int lt_op_rk_stage(const void* y_dev, const void* const* k_ptrs_host, const float* coef_host, int32_t nk, float dt, void* out_dev,
                              int64_t n, int32_t dtype, void* stream) {
    return launch_rk_stage(y_dev, k_ptrs_host, coef_host, nk, dt, out_dev, (long long)n, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_rk_error_norm(const void* y_dev, const void* y1_dev, const void* const* k_ptrs_host, const float* coef_host, int32_t nk,
                                   float dt, float rtol, float atol, void* q_dev, void* ws_dev, float* norm_dev, int64_t n, int32_t dtype,
                                   void* stream) {
    return launch_rk_error_norm(y_dev, y1_dev, k_ptrs_host, coef_host, nk, dt, rtol, atol, q_dev, ws_dev, norm_dev, (long long)n, dtype,
                                (hipStream_t)stream);
}
extern "C" int lt_op_rk_dense(const void* y_dev, const void* y1_dev, const void* ymid_dev, const void* fy_dev, const void* f1_dev, float dt,
                              void* c1_dev, void* c_dev, void* b_dev, void* a_dev, int64_t n, int32_t dtype, void* stream) {
    return launch_rk_dense(y_dev, y1_dev, ymid_dev, fy_dev, f1_dev, dt, c1_dev, c_dev, b_dev, a_dev, (long long)n, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_rk_interp(const void* const* coef_ptrs_host, float x, void* out_dev, int64_t n, int32_t dtype, void* stream) {
    return launch_rk_interp(coef_ptrs_host, x, out_dev, (long long)n, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_rms_norm(const void* x_dev, const void* sub_dev, const void* y0_dev, float rtol, float atol, void* q_dev, void* ws_dev,
                              float* norm_dev, int64_t n, int32_t dtype, void* stream) {
    return launch_rms_norm(x_dev, sub_dev, y0_dev, rtol, atol, q_dev, ws_dev, norm_dev, (long long)n, dtype, (hipStream_t)stream);
}

// ---- the boundary kernels of a model evaluation (misc.hip) and the stand-alone space router (moe.hip) for tests/test_gpu_misc_exact.py: every
// argument of the launcher, unchanged, plus the stream ----------------------------------------------------------------------------------------
extern "C" int lt_op_patchify(const void* x, int32_t x_dtype, void* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t patch, int32_t kpad,
                              int32_t dup_first_half, int32_t wp_stride, void* stream) {
    return launch_patchify(x, x_dtype, (u16*)out, B, C, H, W, patch, kpad, dup_first_half, wp_stride, (hipStream_t)stream);
}
extern "C" int lt_op_eol_fill(void* x, const void* eol, int32_t rows_total, int32_t Wp, int32_t d, void* stream) {
    return launch_eol_fill((u16*)x, (const u16*)eol, rows_total, Wp, d, (hipStream_t)stream);
}
extern "C" int lt_op_fill_rows_bf16(void* dst, const void* row, int64_t rows, int32_t d, void* stream) {
    return launch_fill_rows_bf16((u16*)dst, (const u16*)row, (long long)rows, d, (hipStream_t)stream);
}
extern "C" int lt_op_label_gather(const void* table, const void* labels, void* out, int32_t B, int32_t rows, int32_t d, void* stream) {
    return launch_label_gather((const u16*)table, (const int32_t*)labels, (u16*)out, B, rows, d, (hipStream_t)stream);
}
extern "C" int lt_op_cast_to_bf16(const void* src, int32_t dtype, void* dst, int64_t n, void* stream) {
    return launch_cast_to_bf16(src, dtype, (u16*)dst, (long long)n, (hipStream_t)stream);
}
extern "C" int lt_op_upload_rows(const void* src, int32_t dtype, void* dst, int32_t rows, int32_t cols, int32_t dst_ld, int32_t r0, int32_t row_map,
                                 void* stream) {
    return launch_upload_rows(src, dtype, (u16*)dst, rows, cols, dst_ld, r0, row_map, (hipStream_t)stream);
}
extern "C" int lt_op_mask_to_bias(const void* mask, void* bias, int32_t B, int32_t T, int32_t Tpad, void* stream) {
    return launch_mask_to_bias((const int32_t*)mask, (float*)bias, B, T, Tpad, (hipStream_t)stream);
}
extern "C" int lt_op_add_bf16(const void* a, const void* b, void* c, int64_t n, void* stream) {
    return launch_add_bf16((const u16*)a, (const u16*)b, (u16*)c, (long long)n, (hipStream_t)stream);
}
extern "C" int lt_op_timestep_features(const void* t, int32_t t_index, void* out, int32_t B, int32_t dim, void* stream) {
    return launch_timestep_features((const float*)t, t_index, (u16*)out, B, dim, (hipStream_t)stream);
}
extern "C" int lt_op_cap_pool_ln(const void* cap, int32_t cap_dtype, const void* mask, const void* ln_w, const void* ln_b, void* out, int32_t B,
                                 int32_t T, int32_t C, void* stream) {
    return launch_cap_pool_ln(cap, cap_dtype, (const int32_t*)mask, (const u16*)ln_w, (const u16*)ln_b, (u16*)out, B, T, C, (hipStream_t)stream);
}
extern "C" int lt_op_unpatchify_cfg(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H,
                                    int32_t W, int32_t patch, int32_t use_cfg, float cfg_scale, int32_t cfg_channels, int32_t wp_stride,
                                    void* stream) {
    return launch_unpatchify_cfg((const u16*)rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, use_cfg, cfg_scale, cfg_channels, wp_stride,
                                 (hipStream_t)stream);
}
extern "C" int lt_op_unpatchify_cfg_dev(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H,
                                        int32_t W, int32_t patch, int32_t use_cfg, const float* cfg_scale_dev, int32_t cfg_channels,
                                        int32_t wp_stride, int32_t dup, void* stream) {
    return launch_unpatchify_cfg_dev((const u16*)rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, use_cfg, cfg_scale_dev, cfg_channels, wp_stride,
                                     dup, (hipStream_t)stream);
}
extern "C" int32_t lt_op_guidance_slices(void) { return LT_GUIDANCE_SLICES; }
extern "C" int lt_op_guidance_stats(const void* rows, int32_t ld, int32_t B, int32_t out_ch, int32_t H, int32_t W, int32_t patch,
                                    const float* cfg_scale_dev, int32_t cfg_channels, int32_t wp_stride, double* partials_dev, void* stream) {
    return launch_guidance_stats((const u16*)rows, ld, B, out_ch, H, W, patch, cfg_scale_dev, cfg_channels, wp_stride, partials_dev, (hipStream_t)stream);
}
extern "C" int lt_op_unpatchify_cfg_rule(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H,
                                         int32_t W, int32_t patch, int32_t use_cfg, const float* cfg_scale_dev, int32_t cfg_channels,
                                         int32_t wp_stride, int32_t dup, const double* partials_dev, const float* rescale_dev,
                                         const float* norm_limit_dev, float* factor_out_dev, void* stream) {
    return launch_unpatchify_cfg_rule((const u16*)rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, use_cfg, cfg_scale_dev, cfg_channels, wp_stride,
                                      dup, partials_dev, rescale_dev, norm_limit_dev, factor_out_dev, (hipStream_t)stream);
}
extern "C" int lt_op_guidance_project_stats(const void* rows, int32_t ld, int32_t B, int32_t out_ch, int32_t H, int32_t W, int32_t patch,
                                            int32_t cfg_channels, int32_t wp_stride, int32_t form, const float* par_dev, float* mom_dev,
                                            double* partials_dev, void* stream) {
    return launch_guidance_project_stats((const u16*)rows, ld, B, out_ch, H, W, patch, cfg_channels, wp_stride, form, par_dev, mom_dev, partials_dev,
                                         (hipStream_t)stream);
}
extern "C" int lt_op_unpatchify_cfg_project(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch,
                                            int32_t H, int32_t W, int32_t patch, int32_t use_cfg, const float* cfg_scale_dev, int32_t cfg_channels,
                                            int32_t wp_stride, int32_t dup, int32_t form, const double* partials_dev, const float* par_dev,
                                            const float* mom_dev, float* coef_out_dev, void* stream) {
    return launch_unpatchify_cfg_project((const u16*)rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, use_cfg, cfg_scale_dev, cfg_channels,
                                         wp_stride, dup, form, partials_dev, par_dev, mom_dev, coef_out_dev, (hipStream_t)stream);
}
extern "C" int lt_op_unpatchify_cfg_reuse(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H,
                                          int32_t W, int32_t patch, const float* cfg_scale_dev, int32_t cfg_channels, int32_t wp_stride,
                                          void* delta_dev, int32_t mode, void* stream) {
    return launch_unpatchify_cfg_reuse((const u16*)rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, cfg_scale_dev, cfg_channels, wp_stride,
                                       (u16*)delta_dev, mode, (hipStream_t)stream);
}
extern "C" int lt_op_unpatchify_cfg_slg(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H,
                                        int32_t W, int32_t patch, const float* cfg_scale_dev, const float* slg_scale_dev, int32_t cfg_channels,
                                        int32_t wp_stride, void* skip_dev, int32_t mode, void* stream) {
    return launch_unpatchify_cfg_slg((const u16*)rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, cfg_scale_dev, slg_scale_dev, cfg_channels,
                                     wp_stride, (u16*)skip_dev, mode, (hipStream_t)stream);
}
extern "C" int32_t lt_op_cache_ws_bytes(void) { return (int32_t)(2 * LT_CACHE_BLOCKS * sizeof(double)); }
extern "C" int lt_op_cache_indicator(const void* h_dev, void* h_prev_dev, int64_t n, void* ws_dev, double* sums_dev, void* stream) {
    return launch_cache_indicator((const u16*)h_dev, (u16*)h_prev_dev, (long long)n, (double*)ws_dev, sums_dev, (hipStream_t)stream);
}
extern "C" int lt_op_cache_residual_store(const void* xl_dev, const void* x0_dev, void* r_dev, int64_t n, void* stream) {
    return launch_cache_residual_store((const u16*)xl_dev, (const u16*)x0_dev, (u16*)r_dev, (long long)n, (hipStream_t)stream);
}
extern "C" int lt_op_cache_residual_apply(void* x_dev, const void* r_dev, const void* scale1p_dev, const void* shift_dev, int32_t ld_mod, void* h_dev,
                                          int32_t B, int32_t N, int32_t d, void* stream) {
    LT_REQUIRE(B >= 1 && N >= 1 && d >= 8 && ld_mod >= d, "lt_op_cache_residual_apply: bad shape");
    return launch_cache_residual_apply((u16*)x_dev, (const u16*)r_dev, (const u16*)scale1p_dev, (const u16*)shift_dev, ld_mod, (u16*)h_dev, B * N, N, d,
                                       (hipStream_t)stream);
}
extern "C" int lt_op_region_text_combine(void* out, const void* txt, const void* gate, int32_t Y, int32_t N, int32_t H, int32_t hd, int32_t Hp,
                                         int32_t Wp, int32_t h_split, int32_t w_split, void* stream) {
    return launch_region_text_combine((u16*)out, (const u16*)txt, (const u16*)gate, Y, N, H, hd, Hp, Wp, h_split, w_split, (hipStream_t)stream);
}
extern "C" int lt_op_ode_combine(int32_t mode, const void* y0, const void* k1, const void* k2, const void* k3, const void* k4, void* out,
                                 int32_t dtype, float dt, int64_t n, void* stream) {
    return launch_ode_combine(mode, y0, k1, k2, k3, k4, out, dtype, dt, (long long)n, (hipStream_t)stream);
}
extern "C" int lt_op_ode_multistep(const void* y_prev, const void* const* k, int32_t nslopes, const float* a, const float* b, int32_t has_corr,
                                   void* y_out, void* p_out, int64_t n, int32_t dtype, void* stream) {
    return launch_ode_multistep(y_prev, k, nslopes, a, b, has_corr, y_out, p_out, (long long)n, dtype, (hipStream_t)stream);
}
extern "C" int lt_op_ode_combine_masked(int32_t mode, const void* y0, const void* k1, const void* k2, const void* k3, const void* k4,
                                        const void* mask, const void* x1, const void* noise, void* out, int32_t dtype, float dt, float t,
                                        float one_minus_t, int64_t n, void* stream) {
    return launch_ode_combine_masked(mode, y0, k1, k2, k3, k4, mask, x1, noise, out, dtype, dt, t, one_minus_t, (long long)n, (hipStream_t)stream);
}
extern "C" int lt_op_rope_table(void* out, int32_t len, int32_t hd, int32_t step, float theta0, float lin0, float theta1, float lin1,
                                int32_t lin_on_pos, void* stream, void* out_t) {
    return launch_rope_table((float*)out, len, hd, step, theta0, lin0, theta1, lin1, lin_on_pos, (hipStream_t)stream, (float*)out_t);
}
extern "C" int lt_op_linear_small_m_ext(const void* a, const void* w, const void* b, void* y, int32_t M, int32_t N, int32_t K, int32_t act_in,
                                        const void* t, const void* a2, int32_t pm_L, int32_t pm_chunks, int32_t pm_d, int32_t pm_final,
                                        uint32_t pm_tanh, uint32_t pm_scale, void* stream) {
    LinearSmallMExtra x;
    x.t = (const float*)t; x.a2 = (const u16*)a2; x.pm_L = pm_L; x.pm_chunks = pm_chunks; x.pm_d = pm_d; x.pm_final = pm_final;
    x.pm_tanh = pm_tanh; x.pm_scale = pm_scale;
    return launch_linear_small_m_ext((const u16*)a, (const u16*)w, (const u16*)b, (u16*)y, M, N, K, act_in, x, (hipStream_t)stream);
}
// the fields of MoeArgs the router reads (x, gate_w, forced, rows, d, E; rows_per_sample and max_tiles for the shared shape check) and writes (sel, wts)
extern "C" int lt_op_moe_route(const void* x, const void* gate_w, const void* forced, int32_t rows, int32_t rows_per_sample, int32_t d, int32_t E,
                               void* sel, void* wts, int32_t max_tiles, void* stream) {
    MoeArgs m;
    m.x = (const u16*)x; m.gate_w = (const u16*)gate_w; m.sample_logits = nullptr; m.forced = (const int*)forced;
    m.rows = rows; m.rows_per_sample = rows_per_sample; m.d = d; m.E = E;
    m.sel = (int*)sel; m.wts = (u16*)wts; m.pos = nullptr; m.src = nullptr; m.tile_expert = nullptr; m.max_tiles = max_tiles;
    return launch_moe_route(m, (hipStream_t)stream);
}

// ---- the ragged boundary kernels of a packed batch (packed.hip) for tests/test_gpu_packed_ops.py.  hw_host = [B][2] latent sizes; the entry
// builds the table, stores it at tab_dev (LT_PK_ROWS * LT_PK_MAX ints of device memory) and launches the kernel on it.  N = token rows per sample.
extern "C" int lt_op_packed_table(const int32_t* hw_host, int32_t B, int32_t C, int32_t patch, int32_t* table_host, int64_t* elems, int32_t* n_max) {
    LT_REQUIRE(hw_host && table_host, "lt_op_packed_table: null argument");
    PackedTable t;
    long long n = 0;
    int nm = 0;
    if (int rc = packed_table_build(hw_host, B, C, patch, &t, &n, &nm, nullptr, nullptr)) return rc;
    memcpy(table_host, t.v, sizeof(t.v));
    if (elems) *elems = n;
    if (n_max) *n_max = nm;
    return 0;
}
namespace {
int packed_op_table(const char* who, const int32_t* hw_host, int B, int C, int patch, int N, void* tab_dev, hipStream_t s) {
    LT_REQUIRE(hw_host && tab_dev, "%s: null argument", who);
    PackedTable t;
    int nm = 0;
    if (int rc = packed_table_build(hw_host, B, C, patch, &t, nullptr, &nm, nullptr, nullptr)) return rc;
    LT_REQUIRE(N >= nm, "%s: %d token rows per sample, the longest sample has %d", who, N, nm);
    return launch_packed_table_store(t, (int*)tab_dev, s);
}
}  // namespace
extern "C" int lt_op_patchify_packed(const void* x_flat, int32_t x_dtype, void* out, const int32_t* hw_host, void* tab_dev, int32_t B, int32_t C,
                                     int32_t patch, int32_t kpad, int32_t N, int32_t dup_first_half, void* stream) {
    if (int rc = packed_op_table("lt_op_patchify_packed", hw_host, B, C, patch, N, tab_dev, (hipStream_t)stream)) return rc;
    if (dup_first_half)
        for (int b = 0; b < B / 2; ++b)
            LT_REQUIRE(hw_host[2 * b] == hw_host[2 * (b + B / 2)] && hw_host[2 * b + 1] == hw_host[2 * (b + B / 2) + 1],
                       "lt_op_patchify_packed: samples %d and %d of the two halves differ in size", b, b + B / 2);
    return launch_patchify_packed(x_flat, x_dtype, (u16*)out, (const int*)tab_dev, B, C, patch, kpad, N, dup_first_half, (hipStream_t)stream);
}
extern "C" int lt_op_fill_pad_packed(void* x, const void* pad_token, const int32_t* hw_host, void* tab_dev, int32_t B, int32_t patch, int32_t N,
                                     int32_t d, void* stream) {
    if (int rc = packed_op_table("lt_op_fill_pad_packed", hw_host, B, 1, patch, N, tab_dev, (hipStream_t)stream)) return rc;
    return launch_fill_pad_packed((u16*)x, (const u16*)pad_token, (const int*)tab_dev, B, N, d, (hipStream_t)stream);
}
extern "C" int lt_op_unpatchify_packed(const void* rows, int32_t ld, void* out_flat, int32_t out_dtype, const int32_t* hw_host, void* tab_dev,
                                       int32_t B, int32_t C, int32_t out_ch, int32_t patch, int32_t N, int32_t use_cfg, float cfg_scale,
                                       int32_t cfg_channels, void* stream) {
    if (int rc = packed_op_table("lt_op_unpatchify_packed", hw_host, B, C, patch, N, tab_dev, (hipStream_t)stream)) return rc;
    if (use_cfg)
        for (int b = 0; b < B / 2; ++b)
            LT_REQUIRE(hw_host[2 * b] == hw_host[2 * (b + B / 2)] && hw_host[2 * b + 1] == hw_host[2 * (b + B / 2) + 1],
                       "lt_op_unpatchify_packed: samples %d and %d of the two halves differ in size", b, b + B / 2);
    return launch_unpatchify_packed((const u16*)rows, ld, out_flat, out_dtype, (const int*)tab_dev, B, C, out_ch, patch, N, use_cfg, cfg_scale,
                                    cfg_channels, (hipStream_t)stream);
}
