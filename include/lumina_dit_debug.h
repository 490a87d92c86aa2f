/* lumina_dit_debug.h - A/B options and diagnostics of the MI355X (gfx950) Next-DiT denoising engine.
 *
 * NOT part of the drop-in boundary (include/lumina_dit.h): nothing here is needed to run the reference's path.  This header names
 * the options lt_set_option / lt_engine_set_option accept (A/B measurements, tests; every default is the measured-best setting) and
 * declares the instrumented-kernel entry point and the row kernels' full-argument test entry points.  The option table itself lives in lumina-t2x_amd/csrc/options.hip;
 * tests/test_abi.py keeps this text and the table in step (every name, its range and default).
 *
 * Threads.  The promise of lumina_dit.h - two engines can be driven from two threads - covers the ENGINE entry points only.  The operator
 * entry points (lt_op_*) share process-wide scratch space: the head_dim-96 attention's tail-split workspace is ONE buffer per device for
 * every stream (csrc/attention_v4_96.hip, own_tail_ws).  Op-level entries must not run concurrently on two streams of one device, from one
 * thread or from several; calls on one stream at a time, from any thread, are fine.
 */
#ifndef LUMINA_DIT_DEBUG_H
#define LUMINA_DIT_DEBUG_H

#include "lumina_dit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Options - name (range, default): meaning.
 *   "graph"             (0..2, 2): 1 one model evaluation is captured into a HIP graph per (shape, arguments, option generation) and replayed
 *                       | 2 the same above 1024 rows only: at 512 rows plain launches are 1.5-4.6 % faster (round 5 same-box A/B) | 0: eager
 *                       launches
 *   "attention_variant" (1..6, 4): 1 baseline | 2 VALU-diet | 3 ping-pong wave groups (hd 72 / 96) | 4 one wave per SIMD x 64 query
 *                       rows, asm-owned AGPRs (hd 72, 96 and 48 with whole 64-key tiles; variant 3 otherwise) | 6 = 4 with the hd-48
 *                       one-wave kernel forced at every size | 5 is refused (the PV-on-16x16x32 study kernel, removed in round 5)
 *   "qkv_post_fused"    (0..2, 2): 2 one launch for q / k post-processing + V transpose below 2048 rows (launch-bound regime), three
 *                       launches above | 1 always one launch | 0 always separate launches
 *   "qkv_vt_epilogue"   (0..1, 1): the V projection's epilogue writes the attention kernels' transposed, key-permuted V image directly
 *                       (no V transpose pass; needs tokens per sample % 64 == 0, large M) | 0: off
 *   "qkv_fused_gemm"    (0..1, 1): Q | K | V projection in one launch where the shapes are whole 256 x 288 (or 256 x 256) tiles
 *   "qk_post_pair"      (0..1, 1): q and k post-processing share one persistent launch (>= 2048 rows) | 0: two launches
 *   "attn_q_fused"      (0..1, 1): behind the fused QKV launch at head_dim 72 (2-D RoPE, qk_norm, whole 64-key tiles) q_norm + RoPE of
 *                       the queries happen in the attention kernel's prologue - the QKV GEMM's epilogue leaves per-row LayerNorm partial
 *                       sums, the K pass reduces them to (mean, rstd) - and q is never written head-major; the row statistics come from
 *                       (sum, sum of squares) instead of the two-pass form, so a few queries differ by one bf16 ulp from the "0" path
 *   "norm_specialize"   (0..1, 1): gated_residual_norm runs instantiations with its three mode switches fixed at compile time (the
 *                       engine's combinations at d = 1536 / 2304 / 3072; bit-identical, 34.4 -> 31.6 us) | 0: generic kernel
 *   "gemm_w4q"          (0..1, 1): large dense GEMMs run on the persistent 4-wave 16x16x32 kernel | 0: classic / ping-pong tiles
 *   "gemm_prefetch"     (0..3, 3): 3 at <= 1024 rows the weight panels of the QKV / O / W1|W3 projections are read into the L2 of the
 *                       XCDs that will stage them by extra workgroups of the row kernel in front of the GEMM | 0 off | 1 a serial
 *                       prefetch launch in front of every small-M GEMM (the upper-bound measurement form) | 2 is refused (the
 *                       side-stream form lost 33 % and was removed in round 5)
 *   "gemm_splitk"       (0..2, 1): 1 the 64 x 128 small-M tile splits K over two workgroups per tile when both halves fit one round of
 *                       the CUs (the 512-row O / W2 projections) | 2 whenever the workspace allows | 0 off
 *   "gemm_w4q_grouped"  (0..2, 1): 1 the grouped (mixture-of-experts) GEMMs run on the persistent kernel's grouped mode from 1.5 tiles
 *                       of 256 x 256 per CU on | 2 from 2 tiles per CU on (A/B) | 0 always the 8-wave ping-pong / classic tiles
 *   "gemm_group"        (0..64, 0): tile rows per group of the XCD-aware tile order, 0 = the built-in 4 (experiment, no measured effect)
 *   "gemm_stagger"      (0..256, 0): the persistent 4-wave GEMM kernels spread the start of the workgroups of an XCD over eight phases,
 *                       n * ~256 cycles apart (experiment: de-synchronises the tile-end store bursts; measured -0.5 % .. 0 by box)
 *   "gemm_variant"      (0..2, 0): tile shape of the classic kernels when the caller passes variant 0: 0 auto | 1 256x256 | 2 256x288
 *   "rmsnorm_apex"      (0..1, 0): rounding order of the weighted RMSNorms.  0 = the reference's vanilla class
 *                       (lumina_next_t2i/models/components.py:11-54): bf16(x * rstd) * w, two roundings.  1 = apex.FusedRMSNorm, which
 *                       the reference uses when apex is importable (components.py:6-9): bf16(x * rstd * w), the weight applied in fp32
 *                       before the one rounding - as SURVEY.md 8c describes it; DESIGN.md 6 explains why the default order is expected to
 *                       match an apex box too.  Meant for the text-conditional families (Next-DiT T2I, Flag-DiT: the only ones whose
 *                       reference imports apex) - set it per engine (lt_engine_set_option) and before lt_prepare_prompt, whose hoisted
 *                       text K / V go through the same norm
 *   "attn_small_fused"  (0..1, 1): class-conditional models at head_dim 48 and <= 512 tokens (the 600M ImageNet / MoE models at 256^2): q_norm,
 *                       k_norm, RoPE, the V transpose and the attention itself are ONE launch that reads the QKV projection's output and the
 *                       per-tile LayerNorm partials its GEMM epilogue left (round 5: one launch boundary less per layer where every launch
 *                       is latency-bound) | 0: q / k / v post-processing launch + attention launch
 *   "moe_route_fused"   (0..1, 1): Next-DiT-MoE with both MoE layers per block (models2.py): the row kernel between the time and the space layer
 *                       (combine + gated residual + pre-norm) also routes the space layer - it has the router's input row in registers:
 *                       bf16 logits, top-2, fp32 softmax, bf16 weights, moe_route_kernel's arithmetic statement for statement, bit-identical
 *                       selections (round 5: one launch less per layer) | 0: a separate routing launch
 *   "gemm_splitk4"      (0..1, 1): with "gemm_splitk" on, a dense small-M plain-epilogue GEMM with K >= 4096 (the 512-row w2 projection) runs on
 *                       128 x 128 tiles with K split FOUR ways when that still fits one round of the CUs; the last arriver sums the four
 *                       fp32 partials in K order (round 5) | 0: the two-way split on 64 x 128 tiles
 *   "moe_time_plan_hoist" (0..1, 1): the time-routed MoE layers' plans (selection, weights, expert-sorted positions, tile table) of ALL layers
 *                       are written by one launch at the top of the evaluation - the time router's logits depend on the timestep embedding
 *                       only and are already computed there for every layer (round 5: one launch less per layer); not used while routing is
 *                       forced by the parity hook or with more than 64 samples | 0: one plan launch per layer
 *   "grn_ystat"         (0..2, 1): the O and W2 projections (persistent kernel, plain dense tiles) leave the per-row sum of squares of their
 *                       outputs behind, in partial sums per column tile and wave half, and the sandwich-norm row kernel that follows runs
 *                       its streaming form on it (64 registers, all rows resident; round 6) | 2: the same with two rows per wave (the second row's loads
 *                       in flight under the first row's arithmetic and stores) | 0: the row kernel loads the row, reduces, applies
 *   "qk_wg_per_cu"      (1..8, 3): persistent 4-wave workgroups per CU of the stand-alone q / k post-processing launch (LayerNorm + RoPE + head-major
 *                       view; at cfg 2 the K rows of a layer: 8192 rows over 3 x 256 x 4 waves = 2.67 rows per wave)
 *   "prologue_fused"    (0..7, 0): bit mask - 1: the timestep features are formed inside the first t_embedder GEMV, 2: temb + caption / label
 *                       embedding inside the adaLN GEMV, 4: the per-NFE gate / scale preparation as that GEMV's epilogue; each removes one launch
 *                       and is bit-identical to the separate kernel, and each measured SLOWER than the launch it removes (round 6,
 *                       profiles/r06/bench_ab_prologue_merges_cfg1_cfg5_all_lose.log) | 0 (default): the separate kernels
 *   "gemm_tail_split"   (0..2, 0): 1: the experts' W2 GEMM on the grouped persistent kernel cuts the tiles of a partial last round of its walk
 *                       along K into 2 / 4 parts (the MoE at 1024^2: 1.5-1.6 rounds of 256 x 256 tiles run as 2); the last part of a tile to
 *                       arrive sums the fp32 parts in K order | 2: two-way splits only | 0 (default): whole tiles only.  Built for VERDICT r5
 *                       item 5b and measured SLOWER (cfg5-1024: 24.73 -> 26.8 ms four-way, 24.95 two-way): a 256 x 256 fp32 part is 256 KB
 *                       through a CU that moves ~50-100 GB/s - the hand-off costs what the split saves (profiles/r06)
 *   "attn_text_skip"    (0..1, 1): the one-wave attention kernels (head_dim 72 / 96) do not run text tiles behind a sample's last valid text
 *                       key (the unconditional half of a CFG pair: 8 valid keys of 128 -> one 64-key tile instead of two); the skipped keys
 *                       are all masked, so results are bit-identical (round 6) | 0: every text tile up to Tk
 *   "attn_tail_split"   (0..4, 4): head_dim 96 one-wave kernel, sequences with a partial last query block of 64 or 128 rows (Flag-DiT at
 *                       1024^2: 4160 tokens = 16 x 256 + 64, the 64 workgroups of a fifth round with one live wave each): that block runs as
 *                       this many workgroups over disjoint key ranges ((O^T, m, l) partials in fp32) and a merge launch writes its rows
 *                       (round 6) | 0, 1: one workgroup per block as before
 *   "pair_layout"       (0..1, 1): evaluations whose dense blocks run all four GEMMs on the persistent kernel (the fused QKV launch, O, W1 | W3,
 *                       W2: >= one 256-row tile per CU) and the attention on a one-wave kernel keep the GEMMs' A operands (pre-norm output,
 *                       attention output, SwiGLU output) and the four weights of every layer in the row-pair-interleaved layout (lumina_dit.h,
 *                       lt_op_pair_layout): the LDS-DMA stream then fetches whole 128-byte lines - half the requests into the L2, the
 *                       counter that separated this kernel from the vendor's (round 6).  The weights are converted in place when the
 *                       regime changes (a 256-token call after a 4096-token one) and before every lt_set_weight; bit-identical results
 *                       | 0: row-major everywhere.  Packed batches (lt_forward_packed and its kin) take the regime too when their
 *                       attention runs on the head_dim-72 one-wave kernel (longest sequence a multiple of 64).
 *                       lt_engine_get_option(e, "last_pair", &v) - read-only, no option, e != NULL - says whether the engine's last
 *                       evaluation ran in this regime (1) or row-major (0); "layout_flips" - read-only too - is the number of times the
 *                       weights were converted between the two layouts during the engine's last whole-trajectory sampler call (each
 *                       conversion rewrites every GEMM weight once; a guidance schedule that alternates between a 2 B'-row and a B'-row
 *                       evaluation on different sides of the threshold pays it at every change)
 *                       "layout_pinned" - read-only as well - is 1 once an evaluation was recorded on a stream the CALLER was capturing
 *                       (torch.cuda.graph / hipStreamBeginCapture around lt_forward / lt_forward_cfg): that graph holds row-major kernels and
 *                       replays without the engine hearing of it, so from then on, for the engine's life, no evaluation takes the pair
 *                       regime ("last_pair" stays 0), the weights stay row-major and the shared RoPE table is rebuilt before every
 *                       evaluation (the row-major persistent GEMM is the slower one: an engine that is never captured pays
 *                       nothing)
 * (the round-1 names gemm_pipeline / gemm_pp_tail / gemm_persist are accepted with value 0 only: the study kernels they selected were
 *  deleted with csrc/experimental/ in round 5) */

/* diagnostics: the hd-72 self-attention kernels built with clock stamps.  Variant 3 (ping-pong): trace_dev receives, for every 64th
 * workgroup and each of its 8 waves, 8 x uint64: cycle totals of {X phase (MFMA), DMA wait, barrier, Y phase (softmax + DMA issue),
 * barrier}, the tile count.  Variant 4 (one wave per SIMD): per workgroup 8 x uint64 = s_memrealtime (100 MHz) at entry | loop start |
 * loop end | exit, shader clocks of the loop.  Readers: scripts/attn_trace.py, scripts/attn_trace_v4.py. */
int lt_op_attention_trace(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int32_t B,
                          int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad, int32_t hd, float scale,
                          void* trace_dev, void* stream);

/* The row kernels (csrc/norm.hip, csrc/qkv_post.hip) with every argument of their launchers, for tests/test_gpu_rows_exact.py.  Pointer
 * arguments that a form does not use are NULL.  Layouts: lumina_dit.h (lt_op_rmsnorm_mod, lt_op_gated_residual_norm, lt_op_qk_norm_rope,
 * lt_op_v_transpose, lt_op_pair_layout).
 *   out_pair / h_pair: the output in the row-pair-interleaved layout (even row count, d % 32 == 0).
 *   ystat: [B * N][ystat_slots] float partial sums of squares of the rows of y, as a plain input: the streaming kernel without a GEMM.
 *   moe_ys [sorted rows, d], moe_pos int32 [B * N][2], moe_wts bf16 [B * N][2]: y is the top-2 combine formed on load (y may be NULL).
 *   route_w bf16 [route_E, d], route_sel int32 [B * N][2], route_wts bf16 [B * N][2], route_forced int32 [B * N][2] or NULL: the MoE kernel with
 *   next_mode 1 routes h on its way out.
 *   cs_table: [2][cs_len][hd / 4 (rope_mode 1) or hd / 2 (rope_mode 2)] float (cos, sin); branch 0 is read when t[0] < watershed, branch 1
 *   otherwise and when t is NULL.  n_tok_b / grid_w_b: int32 [B] of a packed batch (rows n >= n_tok_b[b] rotate like the sample's last token).
 *   qstat_in: [B * N][qstat_slots] float2 (sum, sum of squares) over qstat_width columns -> qstat_out [B * N] float2 (mean, rstd).
 * lt_op_gated_residual_norm_describe writes the name of the kernel the launcher would pick (the same expressions as the dispatch). */
int lt_op_rmsnorm_mod_ex(const void* x, const void* w, const void* scale, const void* shift, int32_t ld_mod, void* out, int32_t B,
                         int32_t N, int32_t d, float eps, int32_t scale_pre, int32_t out_pair, void* stream);
int lt_op_gated_residual_norm_ex(void* x, const void* y, const void* post_w, const void* gate, int32_t post_mode, int32_t gate_mode,
                                 const void* next_w, const void* next_scale, const void* next_shift, int32_t next_mode, int32_t ld_mod,
                                 void* h, int32_t B, int32_t N, int32_t d, float eps, float eps_next, int32_t scale_pre, int32_t h_pair,
                                 const void* ystat, int32_t ystat_slots, const void* moe_ys, const void* moe_pos, const void* moe_wts,
                                 const void* route_w, int32_t route_E, void* route_sel, void* route_wts, const void* route_forced,
                                 void* stream);
int lt_op_gated_residual_norm_describe(int32_t post_mode, int32_t gate_mode, int32_t next_mode, int32_t d, int32_t has_next_w,
                                       int32_t has_next_scale, int32_t has_next_shift, int32_t scale_pre, int32_t has_ystat,
                                       int32_t ystat_slots, int32_t has_moe, char* out, int32_t cap);
/* The projection half of lt_op_proj_gated_residual_norm (lumina_dit.h) on its own, as the engine launches O and W2 at large M: C[M, N] = A[M, K] W[N, K]^T,
 * the plain dense GEMM, variant 0, no bias, whose epilogue also leaves every row's partial sums of squares in ystat_ws (float [M][*slots_out];
 * GemmArgs::ystat) - so that a closing step lt_op_proj_gated_residual_norm does not have (a shift, next_mode 2, Flag-DiT's form without post-norm)
 * can follow through lt_op_gated_residual_norm_ex with ystat / ystat_slots.  *slots_out = 2 x the column tiles of 288 or 256 the launch runs on;
 * ystat_cap (floats per row of the workspace) >= that.  Refused by name where the problem does not take the persistent kernel's plain dense tiles
 * (fewer than one 256-row tile per CU): nothing would fill ystat.  tests/forward_chain.py */
int lt_op_gemm_ystat(const void* A, const void* W, void* C, void* ystat_ws, int32_t ystat_cap, int32_t M, int32_t N, int32_t K, int32_t* slots_out,
                     void* stream);
int lt_op_qk_norm_rope_ex(const void* src, int32_t ld_src, int32_t col0, const void* ln_w, const void* ln_b, float ln_eps, void* dst,
                          int32_t B, int32_t N, int32_t heads, int32_t hd, int32_t rope_mode, const void* cs_table, int32_t cs_len,
                          const void* t, float watershed, int32_t grid_w, const void* n_tok_b, const void* grid_w_b, float out_scale,
                          const void* qstat_in, void* qstat_out, int32_t qstat_slots, int32_t qstat_width, void* stream);
int lt_op_qk_norm_rope_pair(const void* qkv, int32_t ld, int32_t q_col0, int32_t k_col0, const void* q_ln_w, const void* q_ln_b,
                            const void* k_ln_w, const void* k_ln_b, float ln_eps, void* q_dst, void* k_dst, int32_t B, int32_t N,
                            int32_t heads, int32_t kv_heads, int32_t hd, int32_t rope_mode, const void* cs_table, int32_t cs_len,
                            const void* t, float watershed, int32_t grid_w, const void* n_tok_b, const void* grid_w_b, float q_out_scale,
                            float k_out_scale, void* stream);
int lt_op_qkv_post(const void* qkv, int32_t ld, int32_t q_col0, int32_t k_col0, int32_t v_col0, const void* q_ln_w, const void* q_ln_b,
                   const void* k_ln_w, const void* k_ln_b, float ln_eps, void* q_dst, void* k_dst, void* vt_dst, int32_t B, int32_t N,
                   int32_t Npad, int32_t heads, int32_t kv_heads, int32_t hd, int32_t rope_mode, const void* cs_table, int32_t cs_len,
                   const void* t, float watershed, int32_t grid_w, const void* n_tok_b, const void* grid_w_b, float q_out_scale,
                   float k_out_scale, void* stream);

/* The kernels of lt_sample_ode_adaptive (csrc/ode_adaptive.hip, where the rounding points are written out) on caller-owned buffers of n
 * elements, any n >= 1; buffers that are not 16-byte aligned take the one-element form.  dtype LT_F32 or LT_BF16 (R: round to dtype).  None reads
 * engine state.  k_ptrs_host: HOST array of nk <= LT_RK_MAX_SLOPES device pointers (the slopes), coef_host their nk coefficients (the fp32 of
 * the tableau's doubles); dt is rounded to dtype by the kernel.  ws_dev: LT_RK_WS_BYTES of device memory, 8-byte aligned; norm_dev: one device
 * float; q_dev (may be NULL) receives the quotients the norm is taken of.
 *   lt_op_rk_stage       out = R(y + R(dt chain(coef)))
 *   lt_op_rk_error_norm  q = R(R(dt chain(coef)) / R(atol + R(rtol max(|y|, |y1|)))),  *norm_dev = fp32(sqrt(mean(q^2)))
 *   lt_op_rk_dense       c1 = R(dt fy) and the dense-output coefficients c, b, a of the step (y, y1, ymid, fy, f1)
 *   lt_op_rk_interp      the quartic through coef_ptrs_host = { y, c1, c, b, a } (HOST array of 5 device pointers) at x
 *   lt_op_rms_norm       *norm_dev = fp32(sqrt(mean(q^2))) in float64, a fixed two-level tree: q = x;  with y0: q = R(x / R(atol + R(|y0| rtol)));
 *                        with sub and y0: q = R(R(x - sub) / scale) */
int lt_op_rk_stage(const void* y_dev, const void* const* k_ptrs_host, const float* coef_host, int32_t nk, float dt, void* out_dev, int64_t n,
                   int32_t dtype, void* stream);
int lt_op_rk_error_norm(const void* y_dev, const void* y1_dev, const void* const* k_ptrs_host, const float* coef_host, int32_t nk, float dt,
                        float rtol, float atol, void* q_dev, void* ws_dev, float* norm_dev, int64_t n, int32_t dtype, void* stream);
int lt_op_rk_dense(const void* y_dev, const void* y1_dev, const void* ymid_dev, const void* fy_dev, const void* f1_dev, float dt, void* c1_dev,
                   void* c_dev, void* b_dev, void* a_dev, int64_t n, int32_t dtype, void* stream);
int lt_op_rk_interp(const void* const* coef_ptrs_host, float x, void* out_dev, int64_t n, int32_t dtype, void* stream);
int lt_op_rms_norm(const void* x_dev, const void* sub_dev, const void* y0_dev, float rtol, float atol, void* q_dev, void* ws_dev, float* norm_dev,
                   int64_t n, int32_t dtype, void* stream);

/* The boundary kernels of a model evaluation (csrc/misc.hip) and the stand-alone space router (csrc/moe.hip), for tests/test_gpu_misc_exact.py.
 * Each entry forwards the arguments of its launcher (csrc/kernels.h, where the layouts are described) unchanged, plus the stream.  dtype
 * arguments: 0 fp32, 1 bf16, 2 fp16 (sources of the casts); the ODE state and the unpatchify output: 0 fp32, 1 bf16.  Pointers are device memory.
 *   linear_small_m_ext: t, a2, pm_L, pm_chunks, pm_d, pm_final, pm_tanh, pm_scale are the fields of LinearSmallMExtra (NULL / 0 / -1: not used).
 *   moe_route: x, gate_w, forced (or NULL), rows, rows_per_sample, d, E are the fields of MoeArgs the router reads, sel and wts the ones it writes;
 *   max_tiles takes part in the launchers' shared shape check only (max_tiles * 256 >= 2 rows + 255 E). */
int lt_op_patchify(const void* x, int32_t x_dtype, void* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t patch, int32_t kpad,
                   int32_t dup_first_half, int32_t wp_stride, void* stream);
int lt_op_eol_fill(void* x, const void* eol, int32_t rows_total, int32_t Wp, int32_t d, void* stream);
int lt_op_fill_rows_bf16(void* dst, const void* row, int64_t rows, int32_t d, void* stream);
int lt_op_label_gather(const void* table, const void* labels, void* out, int32_t B, int32_t rows, int32_t d, void* stream);
int lt_op_cast_to_bf16(const void* src, int32_t dtype, void* dst, int64_t n, void* stream);
int lt_op_upload_rows(const void* src, int32_t dtype, void* dst, int32_t rows, int32_t cols, int32_t dst_ld, int32_t r0, int32_t row_map,
                      void* stream);
int lt_op_mask_to_bias(const void* mask, void* bias, int32_t B, int32_t T, int32_t Tpad, void* stream);
int lt_op_add_bf16(const void* a, const void* b, void* c, int64_t n, void* stream);
int lt_op_timestep_features(const void* t, int32_t t_index, void* out, int32_t B, int32_t dim, void* stream);
int lt_op_cap_pool_ln(const void* cap, int32_t cap_dtype, const void* mask, const void* ln_w, const void* ln_b, void* out, int32_t B, int32_t T,
                      int32_t C, void* stream);
int lt_op_unpatchify_cfg(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H, int32_t W,
                         int32_t patch, int32_t use_cfg, float cfg_scale, int32_t cfg_channels, int32_t wp_stride, void* stream);
/* lt_op_unpatchify_cfg with the scale read from one float of device memory (cfg_scale_dev; may be NULL with use_cfg 0 or dup) and, with dup != 0,
 * the conditional-only form: rows holds B / 2 samples, sample b is written, all channels, to rows b and b + B / 2 of out (use_cfg and the scale
 * play no part).  B counts the rows of out.  Same guidance chain and rounding points as lt_op_unpatchify_cfg. */
int lt_op_unpatchify_cfg_dev(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H, int32_t W,
                             int32_t patch, int32_t use_cfg, const float* cfg_scale_dev, int32_t cfg_channels, int32_t wp_stride, int32_t dup,
                             void* stream);
/* Rescaled / norm-limited guidance (csrc/guidance.hip), for tests/test_gpu_cfg_rule.py.  B counts the 2 B' rows of the evaluation.
 *   guidance_slices: S, the slices a sample's sums are cut into - a constant of the build, the same on every device.
 *   guidance_stats: partials_dev [B' * S * 4] doubles; { sum c, sum c^2, sum g, sum g^2 } of slice s of sample b at [(b * S + s) * 4], over the
 *   first cfg_channels channels of the rows (lt_op_unpatchify_cfg's index walk), g the guided value at the scale in cfg_scale_dev, products and
 *   sums in float64 in an order the launch fixes.  Every one of the B' * S * 4 words is written (an empty slice: zeros), nothing behind them.
 *   unpatchify_cfg_rule: lt_op_unpatchify_cfg_dev with the guided values multiplied in fp32 by the sample's factor f and rounded to bf16; f is
 *   formed in float64 from the partials summed in slice order, the blend in rescale_dev and the limit in norm_limit_dev (one float of device
 *   memory each; +inf: no limit), and rounded once to fp32.  With dup, or with use_cfg 0, the three may be NULL and the result is
 *   lt_op_unpatchify_cfg_dev's.  factor_out_dev (may be NULL): B' floats, the factors.  Refused: an odd B, more than 256 samples. */
int32_t lt_op_guidance_slices(void);
int lt_op_guidance_stats(const void* rows, int32_t ld, int32_t B, int32_t out_ch, int32_t H, int32_t W, int32_t patch, const float* cfg_scale_dev,
                         int32_t cfg_channels, int32_t wp_stride, double* partials_dev, void* stream);
int lt_op_unpatchify_cfg_rule(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H, int32_t W,
                              int32_t patch, int32_t use_cfg, const float* cfg_scale_dev, int32_t cfg_channels, int32_t wp_stride, int32_t dup,
                              const double* partials_dev, const float* rescale_dev, const float* norm_limit_dev, float* factor_out_dev,
                              void* stream);
/* Projected guidance (csrc/guidance_project.hip), for tests/test_gpu_cfg_project.py.  form: LT_PROJECT_APG (1) /
 * LT_PROJECT_ZERO_STAR (2).  B counts the 2 B' rows of the evaluation; S = lt_op_guidance_slices(); par_dev: four floats { scale, eta, beta, r }.
 *   guidance_project_stats: partials_dev [B' * S * 3] doubles, slice s of sample b at [(b * S + s) * 3]: APG { sum m^2, sum m c, sum c^2 } with
 *   m = bf16(c - u) + beta * mom, which REPLACES mom_dev (fp32 [B', cfg_channels, H, W]) word by word; Zero* { sum c u, sum u^2, 0 }, par_dev and
 *   mom_dev may be NULL.  Products and sums in float64 in an order the launch fixes; every one of the B' * S * 3 words is written, nothing behind.
 *   unpatchify_cfg_project: lt_op_unpatchify_cfg_dev whose guided values are APG's bf16(c + (a m + b c)) with m read from mom_dev, or Zero*'s
 *   bf16(s u + w (c - s u)), the coefficients formed in float64 from the partials summed in slice order (lumina_dit.h has the expressions).
 *   coef_out_dev (may be NULL): APG 2 B' floats (a, b) per sample, Zero* B' floats s.  With dup, or use_cfg 0, the result is
 *   lt_op_unpatchify_cfg_dev's and the pointers behind dup may be NULL.  Refused: an odd B, more than 256 samples, another form. */
int lt_op_guidance_project_stats(const void* rows, int32_t ld, int32_t B, int32_t out_ch, int32_t H, int32_t W, int32_t patch, int32_t cfg_channels,
                                 int32_t wp_stride, int32_t form, const float* par_dev, float* mom_dev, double* partials_dev, void* stream);
int lt_op_unpatchify_cfg_project(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H,
                                 int32_t W, int32_t patch, int32_t use_cfg, const float* cfg_scale_dev, int32_t cfg_channels, int32_t wp_stride,
                                 int32_t dup, int32_t form, const double* partials_dev, const float* par_dev, const float* mom_dev,
                                 float* coef_out_dev, void* stream);
/* Guidance reuse (csrc/guidance_reuse.hip), for tests/test_gpu_cfg_reuse.py.  B counts the 2 B' rows of out; delta_dev: bf16
 * [B', cfg_channels, H, W]; the scale is one float of device memory.  mode 0: lt_op_unpatchify_cfg_dev at use_cfg 1, dup 0 on the 2 B' rows,
 * and delta = bf16(c - u) of the channels < cfg_channels is written.  mode 1: rows holds B' samples; the channels < cfg_channels become
 * bf16(bf16(c' - delta) + bf16(scale * delta)), the others pass, sample b is written to rows b and b + B' of out; delta is only read.
 * Refused: a null argument, an odd B, cfg_channels outside 1..C, a mode other than 0 / 1. */
int lt_op_unpatchify_cfg_reuse(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H, int32_t W,
                               int32_t patch, const float* cfg_scale_dev, int32_t cfg_channels, int32_t wp_stride, void* delta_dev, int32_t mode,
                               void* stream);
/* Skip-layer guidance (csrc/guidance_skip.hip), for tests/test_gpu_slg.py.  B counts the 2 B' rows of out; skip_dev: bf16
 * [B', cfg_channels, H, W]; each scale is one float of device memory.  mode 0 (store): rows holds B' samples, the channels < cfg_channels are
 * copied to skip_dev, out is not written (may be null).  mode 1 (guided): rows holds 2 B' samples; with c, u a sample's cond and uncond word
 * and k the stored one the channels < cfg_channels of both halves become bf16(bf16(u + bf16(w bf16(c - u))) + bf16(s bf16(c - k))), the others
 * pass row by row.  mode 2 (cond): rows holds B' samples; bf16(c + bf16(s bf16(c - k))), the others pass, sample b is written to rows b and
 * b + B'.  Refused: a null argument the mode reads, an odd B, cfg_channels outside 1..C, a mode outside 0..2. */
int lt_op_unpatchify_cfg_slg(const void* rows, int32_t ld, void* out, int32_t out_dtype, int32_t B, int32_t C, int32_t out_ch, int32_t H, int32_t W,
                             int32_t patch, const float* cfg_scale_dev, const float* slg_scale_dev, int32_t cfg_channels, int32_t wp_stride,
                             void* skip_dev, int32_t mode, void* stream);
/* Perturbed attention (csrc/attention_identity.hip), for tests/test_gpu_pag.py: self-attention with the attention map replaced
 * by the identity.  src: the row-major QKV projection, [B * N][ld_src] bf16, its V columns at col0 .. col0 + Hkv * hd; out: [B * N][H * hd] bf16,
 *   out[b, n, h, :] = V[b, n, h / (H / Hkv), :]
 * copied word for word (no rounding), row-major or - out_pair 1 - in the row-pair-interleaved layout (lt_op_pair_layout).  16-byte accesses.
 * Refused by name: a null pointer, H % Hkv != 0, a head_dim other than 48 / 72 / 96 / 128, col0 or ld_src no multiple of 8, V columns that
 * leave the row, a pointer not aligned to 16 bytes, out_pair with an odd B * N or H * hd % 32 != 0. */
int lt_op_attention_identity(const void* src, int32_t ld_src, int32_t col0, void* out, int32_t B, int32_t N, int32_t H, int32_t Hkv, int32_t hd,
                             int32_t out_pair, void* stream);
/* Smoothed-energy guidance (csrc/query_blur.hip), for tests/test_gpu_seg.py: the separable 2-D blur of the query image.
 * q, out: bf16 [B, H, N, hd], two buffers (not in place).  grid_w: tokens per grid row, Hp = N / grid_w rows; blur_w <= grid_w: the columns
 * that are image tokens - the others are copied word for word and are nobody's neighbour.  Per (b, h, channel):
 *   mode 0  a[y][x] = sum_{k=-r..r} w[k] q[y][refl(x + k)] in fp32, one fused multiply-add per tap from k = -r upward, starting from 0.f;
 *           out[y][x] = RN_bf16(the same over y on the fp32 a);  refl: -i -> i, n - 1 + i -> n - 1 - i.  taps_dev: 2 r + 1 fp32 words.
 *   mode 1  out[y][x] = RN_bf16(S / n), S the float64 sum of the n = Hp * blur_w words (taps_dev unused, may be NULL).
 * Refused by name with nothing written: a null pointer, a head_dim other than 48 / 72 / 96 / 128, N % grid_w != 0, blur_w outside 1..grid_w,
 * radius outside 0..LT_SEG_MAX_RADIUS, radius >= min(Hp, blur_w) in mode 0, a misaligned pointer (16 bytes; the taps 4), q == out.
 * lt_op_seg_taps: what the engine derives from sigma, on the host - mode (0 taps / 1 mean), radius, and the 2 r + 1 taps (taps_host: room for
 * 2 * LT_SEG_MAX_RADIUS + 1 floats; mode 1 writes none).  Equal to transport/guidance.py: seg_taps word for word.  Refused: sigma <= 0 or NaN. */
int lt_op_query_blur(const void* q, void* out, const float* taps_dev, int32_t B, int32_t H, int32_t N, int32_t hd, int32_t grid_w, int32_t blur_w,
                     int32_t radius, int32_t mode, void* stream);
int lt_op_seg_taps(float sigma, float* taps_host, int32_t* radius, int32_t* mode);
/* Step caching (csrc/step_cache.hip), for tests/test_gpu_teacache.py.  n: bf16 words, a positive multiple of 8; fixed launch
 * geometry, so the sums are a function of the operands alone.
 *   lt_op_cache_indicator: sums_dev[0] = sum |h - h_prev|, sums_dev[1] = sum |h_prev|, every difference and sum in float64; then h_prev <- h.
 *     ws_dev: lt_op_cache_ws_bytes() bytes of scratch.  h and h_prev in one layout (row-major or row-pair: lt_op_pair_layout).
 *   lt_op_cache_residual_store: r = bf16(xl - x0), fp32 from the bf16 words, one rounding.
 *   lt_op_cache_residual_apply: x <- bf16(x + r) in place; h = bf16(LayerNorm(x) * scale1p [+ shift]) - affine-free LayerNorm with eps 1e-6
 *     and the modulate in fp32, one rounding (gated_residual_norm's next_mode 2); scale1p_dev holds bf16(1 + scale), shift_dev may be NULL,
 *     both [B, ld_mod]; rows = B * N. */
/* lt_debug_cache_read: n bf16 words of one of the engine's step-cache buffers to dst_dev, in stream order - which 0: h_prev, 1: x0, 2: r,
 * 3: the token stream e->x, 4: the GEMM input e->h.  Refused: a null argument, buffers not allocated yet, n beyond max_batch * max_tokens * dim. */
int lt_debug_cache_read(lt_engine* e, int32_t which, void* dst_dev, int64_t n, void* stream);
int32_t lt_op_cache_ws_bytes(void);
int lt_op_cache_indicator(const void* h_dev, void* h_prev_dev, int64_t n, void* ws_dev, double* sums_dev, void* stream);
int lt_op_cache_residual_store(const void* xl_dev, const void* x0_dev, void* r_dev, int64_t n, void* stream);
int lt_op_cache_residual_apply(void* x_dev, const void* r_dev, const void* scale1p_dev, const void* shift_dev, int32_t ld_mod, void* h_dev, int32_t B,
                               int32_t N, int32_t d, void* stream);
/* The ragged boundary kernels of a packed batch (csrc/packed.hip): one launch for all samples.  hw_host = [B][2] latent sizes (host); the
 * flat state holds sample b = [C, H_b, W_b] at element offset sum_{j<b} C H_j W_j; N = token rows per sample in the row buffers (>= the longest
 * sequence).  Each launching entry builds the table of the size list, stores it at tab_dev (5 * 64 ints of device memory) and runs its kernel.
 *   packed_table: the host-side table alone - table_host receives 5 rows of 64 ints (element offset, H_b, W_b, token count, grid width; row r
 *   of sample b at [r * 64 + b]), elems the length of the flat state, n_max the longest sequence (each may be NULL).  Needs no device.
 *   patchify_packed: flat state -> out [B * N, kpad]; rows behind a sample's last token are not written.  dup_first_half as lt_op_patchify.
 *   fill_pad_packed: rows ntok_b .. N - 1 of every sample of x [B * N, d] = pad_token [d] (C plays no part: sizes and patch give the counts).
 *   unpatchify_packed: rows [B * N, ld] -> flat state, lt_op_unpatchify_cfg's arithmetic per sample (use_cfg 0: plain, sigma half dropped). */
int lt_op_packed_table(const int32_t* hw_host, int32_t B, int32_t C, int32_t patch, int32_t* table_host, int64_t* elems, int32_t* n_max);
int lt_op_patchify_packed(const void* x_flat, int32_t x_dtype, void* out, const int32_t* hw_host, void* tab_dev, int32_t B, int32_t C,
                          int32_t patch, int32_t kpad, int32_t N, int32_t dup_first_half, void* stream);
int lt_op_fill_pad_packed(void* x, const void* pad_token, const int32_t* hw_host, void* tab_dev, int32_t B, int32_t patch, int32_t N, int32_t d,
                          void* stream);
int lt_op_unpatchify_packed(const void* rows, int32_t ld, void* out_flat, int32_t out_dtype, const int32_t* hw_host, void* tab_dev, int32_t B,
                            int32_t C, int32_t out_ch, int32_t patch, int32_t N, int32_t use_cfg, float cfg_scale, int32_t cfg_channels,
                            void* stream);
int lt_op_region_text_combine(void* out, const void* txt, const void* gate, int32_t Y, int32_t N, int32_t H, int32_t hd, int32_t Hp, int32_t Wp,
                              int32_t h_split, int32_t w_split, void* stream);
int lt_op_ode_combine(int32_t mode, const void* y0, const void* k1, const void* k2, const void* k3, const void* k4, void* out, int32_t dtype,
                      float dt, int64_t n, void* stream);
/* lt_op_ode_combine mode 0 or 4, its result rounded to the state dtype, then the inpainting blend of lt_sample_ode_masked in the same thread:
 * out = R(R(step mask) + R(R(R(noise one_minus_t) + R(x1 t)) R(1 - mask))); mask, x1, noise: n words of the state dtype. */
int lt_op_ode_combine_masked(int32_t mode, const void* y0, const void* k1, const void* k2, const void* k3, const void* k4, const void* mask,
                             const void* x1, const void* noise, void* out, int32_t dtype, float dt, float t, float one_minus_t, int64_t n,
                             void* stream);
/* one step of lt_sample_ode_multistep on n words: y_out = R(y_prev + S(a, k)) (has_corr), p_out = R(y + S(b, k)) from the stored y (has_corr 0:
 * y = y_prev, y_out is not written); k: host array of nslopes device pointers, newest slope first; a, b: 4 host floats each, a sum running up
 * to the last weight that is not 0; S(c, k): acc = R(c_0 k_0), acc = R(acc + R(c_j k_j)).  dtype 0 f32, 1 bf16. */
int lt_op_ode_multistep(const void* y_prev, const void* const* k, int32_t nslopes, const float* a, const float* b, int32_t has_corr, void* y_out,
                        void* p_out, int64_t n, int32_t dtype, void* stream);
int lt_op_rope_table(void* out, int32_t len, int32_t hd, int32_t step, float theta0, float lin0, float theta1, float lin1, int32_t lin_on_pos,
                     void* stream, void* out_t);
int lt_op_linear_small_m_ext(const void* a, const void* w, const void* b, void* y, int32_t M, int32_t N, int32_t K, int32_t act_in, const void* t,
                             const void* a2, int32_t pm_L, int32_t pm_chunks, int32_t pm_d, int32_t pm_final, uint32_t pm_tanh, uint32_t pm_scale,
                             void* stream);
int lt_op_moe_route(const void* x, const void* gate_w, const void* forced, int32_t rows, int32_t rows_per_sample, int32_t d, int32_t E, void* sel,
                    void* wts, int32_t max_tiles, void* stream);
/* lt_op_moe_plan (lumina_dit.h) with every field of MoeArgs (csrc/kernels.h), for tests/test_moe_plan.py and tests/forward_chain.py.
 *   forced: int32 [rows][2] expert ids (0 .. E - 1, two different ones per row) that replace the top-2 choice, or NULL; with sample_logits the
 *   weights are still the softmax of the row's own two logits, and the plan runs on the single-workgroup kernel.
 *   sample_ld: row stride of sample_logits in elements (0 = E).
 *   layers > 1: the all-layers form of the time router's closed-form plan - layer l reads the logit columns [l * E, l * E + E) of every sample
 *   (sample_ld >= layers * E) and writes sel / pos / wts at + l * layer_stride_rows elements (even, >= 2 rows), src at + l * layer_stride_src
 *   (>= 256 max_tiles), tile_expert at + l * layer_stride_tiles (>= max_tiles); words between the layers' slices are not written.  Refused by
 *   the launcher: layers > 1 without sample_logits, with a forced table, with more than 64 samples or with rows that are not whole samples. */
int lt_op_moe_plan_ex(void* sel, const void* sample_logits, int32_t sample_ld, const void* forced, void* wts, int32_t rows,
                      int32_t rows_per_sample, int32_t E, void* pos, void* src, void* tile_expert, int32_t max_tiles, int32_t layers,
                      int64_t layer_stride_rows, int64_t layer_stride_src, int64_t layer_stride_tiles, void* stream);

/* The two attention launches that build their operands themselves, with every argument the engine fills, for tests/test_gpu_prologue_exact.py.
 *   lt_op_attention_qraw_ex = lt_op_attention_qraw (lumina_dit.h) plus the table-branch select - cs_table / cs_table_t hold two branches,
 *   [2][table_len][hd / 4] (cos, sin) and its transpose [2][hd / 4][table_len]; branch 0 is read when t_dev[0] < watershed, branch 1 otherwise
 *   and when t_dev is NULL - and, optionally, the fused text keys of lt_op_attention_fused (tk NULL: none).
 *   lt_op_attention_small: launch_attention_small alone (csrc/kernels.h, AttnSmallArgs: qkv [B * tokens, ld] with the q / k / v column blocks at
 *   q_col0 / k_col0 / v_col0, rowstat [B * tokens][slots] float2 (sum, sum of squares) per 128-column tile, q / k in slots [q_slot0, + q_nslot) /
 *   [k_slot0, + k_nslot), cs_table [2][table_len][hd / 4] (cos, sin), branch as above, out [B, tokens, H * hd]); ln_eps 1e-5, no prefetch rider. */
int lt_op_attention_qraw_ex(const void* qkv_dev, int32_t ld, int32_t q_col0, const void* q_mean_rstd_dev, const void* q_ln_w_dev,
                            const void* q_ln_b_dev, const void* cs_table_dev, const void* cs_table_t_dev, int32_t table_len, int32_t grid_w,
                            const void* t_dev, float watershed, const void* k_dev, const void* vt_dev, const void* tk_dev, const void* tvt_dev,
                            const float* tbias_dev, const void* tgate_dev, int32_t Tk, int32_t Tkpad, void* out_dev, int32_t B, int32_t H,
                            int32_t Hkv, int32_t N, int32_t Nkpad, int32_t hd, void* stream);
/* lt_op_attention_qraw_ex plus per-sample key counts (nk_dev as lt_op_attention_nk, lumina_dit.h).  The combination is REFUSED by name: the
 * prologue takes one grid_w, a packed batch has a grid width per sample (the engine keeps lt_op_qk_norm_rope's per-sample form for Q there).
 * nk_dev NULL: lt_op_attention_qraw_ex.  The entry exists so that tests/test_gpu_attention_nk.py can reach that refusal; nothing else calls it. */
int lt_op_attention_qraw_nk(const void* qkv_dev, int32_t ld, int32_t q_col0, const void* q_mean_rstd_dev, const void* q_ln_w_dev,
                            const void* q_ln_b_dev, const void* cs_table_dev, const void* cs_table_t_dev, int32_t table_len, int32_t grid_w,
                            const void* t_dev, float watershed, const void* k_dev, const void* vt_dev, const void* tk_dev, const void* tvt_dev,
                            const float* tbias_dev, const void* tgate_dev, int32_t Tk, int32_t Tkpad, void* out_dev, int32_t B, int32_t H,
                            int32_t Hkv, int32_t N, int32_t Nkpad, int32_t hd, const int32_t* nk_dev, void* stream);
int lt_op_attention_small(const void* qkv_dev, int32_t ld, int32_t q_col0, int32_t k_col0, int32_t v_col0, const void* rowstat_dev, int32_t slots,
                          int32_t q_slot0, int32_t q_nslot, int32_t k_slot0, int32_t k_nslot, const void* q_ln_w_dev, const void* q_ln_b_dev,
                          const void* k_ln_w_dev, const void* k_ln_b_dev, const void* cs_table_dev, int32_t table_len, int32_t grid_w,
                          const void* t_dev, float watershed, float k_scale, void* out_dev, int32_t B, int32_t H, int32_t Hkv, int32_t tokens,
                          int32_t hd, void* stream);

/* The guided view gather of lt_sample_views_guided (csrc/views.hip, where the chain is written out) on caller-owned buffers: a plain forward of
 * the launcher's arguments.  y, guidance, noise [C, HW]; perm int32 [V][HW], vsign / isign float [V][C] (DEVICE); f0 [V, C, HW] or NULL (stage 0);
 * out [V, C, HW]; coef_host = { ft, f1t, kc, k1c } (HOST); HW a multiple of 4; dtype LT_F32 or LT_BF16.  Indices are clamped into [0, HW). */
int lt_op_views_guided_gather(const void* y_dev, const void* guidance_dev, const void* noise_dev, const int32_t* perm_dev, const float* vsign_dev,
                              const float* isign_dev, const void* f0_dev, void* out_dev, float half_dt, const float* coef_host, int32_t V,
                              int32_t C, int32_t HW, int32_t dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
