// Internal to the host side of the library (engine.hip, samplers.hip): the engine object and what the whole-trajectory samplers need of
// it.  Not a public header - include/lumina_dit.h is the ABI.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/lumina_dit.h"
#include "common.h"
#include "eval_kind.h"
#include "kernels.h"
#include "options.h"

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct LayerW {
    u16 *wqkv = nullptr, *wo = nullptr, *w13 = nullptr, *w2 = nullptr, *wkvy = nullptr;
    u16 *q_norm_w = nullptr, *q_norm_b = nullptr, *k_norm_w = nullptr, *k_norm_b = nullptr;
    u16 *ky_norm_w = nullptr, *ky_norm_b = nullptr, *gate = nullptr;
    u16 *attn_norm1 = nullptr, *attn_norm2 = nullptr, *ffn_norm1 = nullptr, *ffn_norm2 = nullptr, *y_norm = nullptr;
    u16 *ky = nullptr, *vty = nullptr;  // hoisted text K / V^T of the current prompt
    // MoE family (models2.py:731-745): E experts per branch, w13 packed per expert [E][2F, d], w2 [E][d, F]
    u16 *w13_t = nullptr, *w2_t = nullptr, *w13_s = nullptr, *w2_s = nullptr, *gate_t = nullptr, *gate_s = nullptr;
    u16 *norm_time = nullptr, *norm_space = nullptr;
};

struct ProfClass {
    double flops = 0;
    long long launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;
    size_t budget = (size_t)-1;  // bracket at most this many launches with events, count the rest (same launch mix every step)
    long long skip = 0;          // ... starting with launch number `skip` after a reset (a window in the middle of a timed region)
};

// What differs between the reference's model families on this path (everything else is shared code):
//                    NEXT_T2I (model.py:573-662)   NEXT_IMAGENET (models.py:759-833)   FLAG_T2I (lumina_t2i model.py:572-658)
//  adaLN chunks      scale,gate | scale,gate       scale,gate | scale,gate             shift,scale,gate | shift,scale,gate
//  pre-norm weight   attention_norm1 / ffn_norm1   none (PFRMSNorm)                    attention_norm / ffn_norm
//  post-norm         attention_norm2 / ffn_norm2   attention_norm / ffn_norm           none
//  gate              tanh                          tanh                                plain
//  conditioning      text (cross-attn + pooled)    class label embedding               text (cross-attn + pooled)
//  RoPE              2-D, watershed branches       2-D, (rope_scaling, ntk) at once    1-D over the flattened rows, eol tokens
//  final layer       scale                         shift, scale                        shift, scale
struct VariantDesc {
    int chunks;                  // adaLN chunks per layer
    int i_shift[2], i_scale[2], i_gate[2];  // chunk index of {attention, ffn} branch; -1 = absent
    bool pre_w, post, gate_tanh, text, labels, rope_1d, eol;
    int final_chunks;            // 1: scale;  2: shift, scale
};

// Stage times of a whole-trajectory call (samplers.hip).  The host fills a page-locked buffer (an async copy from pageable memory
// synchronises), ONE async copy takes it to the device and evaluation number `call` of a batch of B rows reads dev + call * B.
struct StageTimes {
    float *dev = nullptr, *pinned = nullptr;
    hipEvent_t copied = nullptr;  // the previous call's copy out of `pinned` has executed
    int cap = 0;                  // floats
    int reserve(int count) {
        LT_CHECK_HIP(hipMalloc((void**)&dev, (size_t)count * sizeof(float)));
        LT_CHECK_HIP(hipHostMalloc((void**)&pinned, (size_t)count * sizeof(float), hipHostMallocDefault));
        cap = count;
        return 0;
    }
    int create(int count) {  // lt_create
        if (reserve(count)) return 1;
        LT_CHECK_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        return 0;
    }
    void release() {  // lt_destroy
        if (dev) (void)hipFree(dev);
        if (pinned) (void)hipHostFree(pinned);
        if (copied) (void)hipEventDestroy(copied);
        dev = nullptr; pinned = nullptr; copied = nullptr; cap = 0;
    }
    int ready(int count, hipStream_t s) {
        if (cap < count) {  // beyond lt_create's 1024 times per batch row (a 257-point rk4 grid): the one case in which a sampler synchronises
            LT_CHECK_HIP(hipStreamSynchronize(s));
            if (dev) LT_CHECK_HIP(hipFree(dev));
            if (pinned) LT_CHECK_HIP(hipHostFree(pinned));
            dev = nullptr; pinned = nullptr; cap = 0;
            if (reserve(count)) return 1;
        }
        LT_CHECK_HIP(hipEventSynchronize(copied));  // the previous trajectory's copy has left the staging buffer (normally long ago)
        return 0;
    }
    // room for `count` times and `pinned` free to be written: the buffer to fill (nullptr after lt_set_error); commit sends it on its way
    float* begin(int count, hipStream_t s) { return ready(count, s) ? nullptr : pinned; }
    int commit(int count, hipStream_t s) {
        LT_CHECK_HIP(hipMemcpyAsync(dev, pinned, (size_t)count * sizeof(float), hipMemcpyHostToDevice, s));
        LT_CHECK_HIP(hipEventRecord(copied, s));
        return 0;
    }
};

// What lt_sample_ode_adaptive needs beyond ys / ymid / kbuf, allocated by its first call: three more slopes (dopri5 holds seven), the four
// dense-output coefficients, the norm's partial sums and result word, and the page-locked word the host reads the error ratio from.
struct RkWork {
    void *k[3] = {nullptr, nullptr, nullptr}, *coef[4] = {nullptr, nullptr, nullptr, nullptr}, *ws = nullptr;
    float *norm_dev = nullptr, *norm_host = nullptr;
    int reserve(size_t state_bytes) {
        if (norm_host) return 0;
        for (auto& p : k) LT_CHECK_HIP(hipMalloc(&p, state_bytes));
        for (auto& p : coef) LT_CHECK_HIP(hipMalloc(&p, state_bytes));
        LT_CHECK_HIP(hipMalloc(&ws, LT_RK_WS_BYTES));
        LT_CHECK_HIP(hipMalloc((void**)&norm_dev, 4 * sizeof(float)));
        LT_CHECK_HIP(hipHostMalloc((void**)&norm_host, 4 * sizeof(float), hipHostMallocDefault));
        return 0;
    }
    void release() {  // lt_destroy (also after a reserve that failed half way)
        for (auto& p : k) { if (p) (void)hipFree(p); p = nullptr; }
        for (auto& p : coef) { if (p) (void)hipFree(p); p = nullptr; }
        if (ws) (void)hipFree(ws);
        if (norm_dev) (void)hipFree(norm_dev);
        if (norm_host) (void)hipHostFree(norm_host);
        ws = nullptr; norm_dev = nullptr; norm_host = nullptr;
    }
};

struct lt_engine {
    lt_config cfg;
    LtEngineOptions opts;  // per-engine option overrides (lt_engine_set_option); LT_OPT_INHERIT slots follow the process defaults
    VariantDesc v;
    int d, L, H, Hkv, hd, F, dkv, qkvn, A, cap, nfinal, kpad, chunks, ld_mod;
    std::vector<DevBuf> allocs;
    std::vector<LayerW> lw;
    // globals
    u16 *xemb_w = nullptr, *xemb_b = nullptr, *t0_w = nullptr, *t0_b = nullptr, *t2_w = nullptr, *t2_b = nullptr;
    u16 *capln_w = nullptr, *capln_b = nullptr, *cape_w = nullptr, *cape_b = nullptr, *pad_token = nullptr;
    u16 *adaln_w = nullptr, *adaln_b = nullptr;  // [L*chunks*d + d, A], [L*chunks*d + d]
    u16 *final_w = nullptr, *final_b = nullptr;
    u16 *label_table = nullptr, *eol_token = nullptr;
    int label_rows = 0;
    std::map<std::string, bool> need;
    bool weights_ok = false;
    // round 6: the dense blocks' four GEMM weights (wqkv, wo, w13, w2 of every layer) are held either row-major or in the row-pair-interleaved
    // layout the persistent GEMM reads with whole-line requests (GemmArgs::pair_ab); ensure_weight_layout converts all of them in place when an
    // evaluation needs the other one (a change of regime: >= one tile per CU <-> the small-M kernels).  last_pair: what the last run_forward used.
    bool w_pair = false, last_pair = false;
    // conversions of the weights between the two layouts: since lt_create, and during the last whole-trajectory sampler call
    // (lt_engine_get_option "layout_flips"; DESIGN 7g: a guidance schedule whose two evaluation sizes fall into different regimes)
    long long layout_flips_total = 0, layout_flips = 0;
    // caller capture: the first evaluation recorded on a stream the CALLER is capturing latches layout_pinned for the engine's
    // life - that graph holds row-major kernels and replays without the engine hearing of it, so no evaluation chooses the pair regime any
    // more, and the shared RoPE table is rebuilt before every evaluation (a replay rewrites it behind the host's back).
    // w_pair_dev: 1 while the weights ARE in the pair layout, written in stream order behind every conversion.  A conversion recorded into a
    // caller's graph reads it (launch_pair_layout only_if), so that it converts once however often the graph replays; w_owed: such a
    // conversion was recorded, not run - the next eager call enqueues the same conditional conversion before it trusts w_pair.
    bool layout_pinned = false, w_owed = false;
    int* w_pair_dev = nullptr;
    // workspace
    u16 *x = nullptr, *h = nullptr, *qkv = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *attn = nullptr;
    u16 *o = nullptr, *u = nullptr, *patches = nullptr, *frows = nullptr, *mod = nullptr;
    u16 *tfeat = nullptr, *t1 = nullptr, *temb = nullptr, *cap_ln = nullptr, *cap_emb = nullptr, *adaln_in = nullptr;
    // MoE workspace: expert-sorted rows (moe.hip)
    int E = 0, moe_tiles = 0;
    int moe_mode = 0;  // 0: time + space MoE per block (models2.py), 1: time-routed MoE only (models.py), 2: token-routed only (models1.py)
    u16 *moe_us = nullptr, *moe_ys = nullptr, *moe_logits = nullptr, *moe_wts = nullptr;
    u16* gate_t_all = nullptr;  // [L * E, A]: every layer's time-router weight, contiguous (LayerW::gate_t point into it)
    int *moe_sel = nullptr, *moe_pos = nullptr, *moe_tile_expert = nullptr, *moe_src = nullptr;
    // round 5 (option moe_time_plan_hoist): one plan per layer for the time router, all written by ONE launch at the top of the evaluation
    int *moe_tp_sel = nullptr, *moe_tp_pos = nullptr, *moe_tp_tile_expert = nullptr, *moe_tp_src = nullptr;
    u16* moe_tp_wts = nullptr;
    size_t moe_tp_stride_rows = 0, moe_tp_stride_src = 0;
    bool moe_tp_live = false;  // this evaluation's time plans were hoisted (set by run_forward, read by moe_ffn / moe_y)
    // parity hooks (lt_moe_routing_*): [L][2 branches][max rows][2] expert ids, recorded from / forced onto moe_route_kernel
    int *moe_rec = nullptr, *moe_force = nullptr;
    int moe_rec_on = 0, moe_force_rows = 0, moe_rec_rows = 0;
    int qstat_slots = 32;
    float* qstat = nullptr;  // [rows][qstat_slots] float2: LayerNorm partial sums of the Q columns, written by the fused QKV GEMM (GemmArgs::qstat)
    float* ystat = nullptr;  // [rows][ystat_cap] floats: per-row sum-of-squares partials of the O / W2 projection's output (GemmArgs::ystat -> GatedResArgs::ystat)
    int ystat_cap = 0;
    float* attn_tail_ws = nullptr;  // hd 96 only: partials of the attention launch's split last query block (AttnArgs::tail_ws)
    size_t attn_tail_ws_bytes = 0;
    float* qmr = nullptr;    // [rows] float2 (mean, rstd) of the Q rows, reduced from qstat by the K pass of qk_norm_rope (AttnArgs::q_stat)
    float* rope_tr = nullptr;  // the 2-D rotary table once more as [branch][freq][pos] (AttnArgs::rope_cs_t)
    // split-K workspace of the 512-row-class GEMMs (GemmArgs::splitk_*): 128 tiles = one round of half the CUs
    float* splitk_part = nullptr;
    unsigned* splitk_cnt = nullptr;
    // tail split of the grouped persistent GEMM (GemmArgs::tail_*; MoE engines with >= 4096 rows): fp32 parts + arrival counters
    float* tail_part = nullptr;
    unsigned* tail_cnt = nullptr;
    long long tail_cap_parts = 0;
    int splitk_tiles = 0;
    u16 *capb = nullptr, *capn = nullptr, *kvy = nullptr;
    float* txt_bias = nullptr;
    float* rope = nullptr;
    float rope_scale = -1.f, rope_ntk = -1.f;
    int rope_len = 0;
    int prompt_B = 0, prompt_T = 0, prompt_Tpad = 0;
    int softmax_rule = LT_SOFTMAX_T2I;  // lt_set_softmax_rule: which reference's proportional-attention scale (part of the graph key)
    // ode
    void *ys[2] = {nullptr, nullptr}, *ymid = nullptr, *kbuf[4] = {nullptr, nullptr, nullptr, nullptr};
    StageTimes times;  // stage times of a whole-trajectory call (samplers.hip)
    RkWork rk;         // lt_sample_ode_adaptive
    // compositional (regional) text conditioning (lt_prepare_prompt_regional): Y captions, the first Y-1 belong to regions of
    // the cond row, the last to the uncond row; 0 = off
    int reg_Y = 0, reg_h = 1, reg_w = 1;
    u16* reg_txt = nullptr;    // [Y, max_tokens, d] per-caption text attention outputs
    size_t reg_txt_elems = 0;
    int* reg_qmap = nullptr;   // [max_batch] query batch of each caption
    int* pk_dev = nullptr;     // packed batches: [0,64) token counts, [64,128) grid widths
    int pk_host[128] = {0};
    int* pk_tab = nullptr;     // packed batches on a flat state (lt_forward_cfg_packed / lt_sample_ode_packed): the device PackedTable (kernels.h)
    long long last_nfe = 0;
    long long last_eval_rows = 0;  // lt_last_eval_rows: the rows the last sampler call's evaluations ran, summed
    // multi-view sampling (lt_set_views / lt_sample_views, views.hip): engine-owned tables of the V views over an h x w latent
    int *vw_perm = nullptr, *vw_iperm = nullptr, *vw_hits = nullptr;  // [V][h w], [V][h w], [V h w + 1]
    float *vw_vsign = nullptr, *vw_isign = nullptr;                   // [V][in_channels]
    int vw_V = 0, vw_h = 0, vw_w = 0;
    // tiled (MultiDiffusion) sampling (lt_set_windows / lt_forward_tiled / lt_sample_ode_tiled, tiled.hip): the window table
    // (tw.n = 0: none; it travels as a kernel argument), the engine's copy of the window weights (tw_has_weight false: all ones, not read) and
    // the per-pixel weight sums, and the window rows going into and coming out of the model.  The four buffers are allocated by the first
    // lt_set_windows at their largest size - weights: one window of max_tokens tokens; sums: max_batch / 2 such windows; rows: max_batch such
    // samples - and kept for the engine's life (a graph the caller recorded around lt_forward_tiled holds the pointers).  The composed calls
    // (lt_forward_compose / lt_sample_ode_compose) keep their (K + 1) B' <= max_batch replicated rows and model outputs in tw_in /
    // tw_out, which are exactly that size, and allocate the set the same way when no tiled call has
    WindowTable tw = {};
    bool tw_has_weight = false;
    float *tw_weight = nullptr, *tw_wsum = nullptr;
    int* tw_bad = nullptr;
    void *tw_in = nullptr, *tw_out = nullptr;
    // HIP graphs of one model evaluation (forward_graphed): fixed staging buffers the captured kernels read / write, a private
    // stream to capture on (the caller's stream may be the legacy null stream, which cannot capture), cached executables
    struct GraphTally { double flops[3] = {0, 0, 0}; long long launches[3] = {0, 0, 0}; };  // what one replay stands for, per kernel class
    struct GraphEntry { std::vector<char> key; hipGraphExec_t exec = nullptr; int uses = 0; bool failed = false; bool pair = false; GraphTally tally; };
    GraphTally* tally = nullptr;  // set while a graph is being captured: ProfScope counts into it instead of timing
    std::vector<GraphEntry> graphs;
    void *g_x = nullptr, *g_out = nullptr;
    float* g_t = nullptr;
    // [4]: the guidance scale of an evaluation that reads it from device memory (lt_sample_ode_cfg_schedule), then the rescale blend and the
    // norm limit of a guidance rule (lt_sample_ode_cfg_rule / lt_forward_cfg_rule), then the skip-layer scale
    float* g_cfg = nullptr;
    double* g_stats = nullptr;  // the rule's partial sums: max_batch / 2 samples x LT_GUIDANCE_SLICES x 4 (guidance_stats -> unpatchify_cfg_rule)
    // guidance reuse: d = bfr(cond - uncond) of the last refresh evaluation, bf16 [B', ch, H, W]; max_batch / 2 x in_channels x
    // max_tokens x patch^2 words, allocated by the first call that needs it (ensure_delta) and kept for the engine's life - captured graphs hold
    // the pointer.  delta_sig: { B', H, W, ch } of what it holds, B' = 0: nothing; every lt_prepare_prompt* / lt_prepare_labels call zeroes it
    u16* g_delta = nullptr;
    int delta_sig[4] = {0, 0, 0, 0};
    // skip-layer guidance: the guided channels of the last skip evaluation, bf16 [B', ch, H, W]; sized and allocated like g_delta
    // (ensure_skip_buf).  Written and read inside one entry-point call only, so it carries no signature
    u16* g_skip = nullptr;
    // projected guidance: which two kernels close an LT_KIND_RULE evaluation - 0 the rescale / norm-limit rule, LT_PROJECT_APG,
    // LT_PROJECT_ZERO_STAR.  An argument of the call that travels here to close_forward, as `skip` does: only ProjectScope writes it, and its
    // destructor puts 0 back on every exit path.  Part of the graph key when it is not 0.
    int rule_form = 0;
    // ... its buffers, allocated by the first call that needs them (ensure_project) and kept for the engine's life - captured graphs hold the
    // pointers: APG's momentum, fp32 [B', ch, H, W] (g_delta's element count); the partial sums, max_batch / 2 x LT_GUIDANCE_SLICES x
    // LT_PROJECT_SUMS; the parameter words { scale, eta, beta, r }.  proj_sig: { B', H, W, ch } of what the momentum holds, B' = 0: nothing;
    // every lt_prepare_prompt* / lt_prepare_labels call zeroes it
    float *p_mom = nullptr, *p_par = nullptr;
    double* p_stats = nullptr;
    int proj_sig[4] = {0, 0, 0, 0};
    // the layers THIS call's evaluation leaves out (ascending, distinct, inside 0 .. L-1, not all of them): an argument of the call that
    // travels here to run_forward.  Only SkipScope writes it, and its destructor empties it on every exit path
    std::vector<int32_t> skip;
    // perturbed-attention guidance: the layers THIS call's evaluation runs with the identity in place of their self-attention map
    // (ascending, distinct, inside 0 .. L-1, disjoint from `skip`; may hold every layer).  Kept like `skip`: SkipScope writes and empties it
    std::vector<int32_t> perturb;
    // smoothed-energy guidance: the layers THIS call's evaluation runs with blurred queries in their self-attention (ascending,
    // distinct, inside 0 .. L-1, disjoint from `skip`; may hold every layer; never together with `perturb`).  Kept like `skip`.  blur_mode /
    // blur_radius: what the call's sigma stands for (seg_taps_host), part of the graph key beside the set; the taps themselves are in blur_taps,
    // 2 * LT_SEG_MAX_RADIUS + 1 fp32 words on the device that ensure_blur writes on the call's stream - no part of the key.  q_blur: the blurred
    // query image, the size of q.  Both buffers are allocated by the first call that needs them (ensure_blur) and kept for the engine's life
    std::vector<int32_t> blur;
    int blur_mode = 0, blur_radius = 0;
    float* blur_taps = nullptr;
    u16* q_blur = nullptr;
    // step caching: the modulated input of the first block of the previous evaluation, the token stream before block 0 and the
    // residual r = bfr(x_L - x_0) of the last evaluation that ran the stack - max_batch * max_tokens x d bf16 each; behind them the indicator's
    // partial sums and its two float64 result words, and the page-locked pair the host reads them from.  Allocated by the first call that needs
    // them (ensure_step_cache) and kept for the engine's life - captured graphs hold the pointers.
    // cache_head: { B, H, W, io_dtype, use_cfg } of the step-caching head whose e->x / e->h / e->mod are in place (B = 0: none; every other evaluation
    // overwrites them and says so); cache_res: { B, H, W, use_cfg } of what c_r holds (B = 0: nothing; every prepare call forgets it)
    u16 *c_hprev = nullptr, *c_x0 = nullptr, *c_r = nullptr;
    double *c_ws = nullptr, *c_sums_host = nullptr;
    int cache_head[5] = {0, 0, 0, 0, 0}, cache_res[4] = {0, 0, 0, 0};
    long long last_cache_hits = 0;  // lt_last_cache_hits: the evaluations of the last lt_sample_ode_cached call that reused the residual
    hipStream_t cap_stream = nullptr;
    long long graph_replays = 0;
    // profiling
    int prof_mask = 0;  // bit k: class k launches are bracketed by HIP events
    bool prof_on = false;
    ProfClass prof[3];
};

// A packed batch on one flat state buffer (packed.hip): what an evaluation needs of the size list.  The device table e->pk_tab holds the
// same list (packed_call_begin stored it on the call's stream).
struct PackedCall {
    const int32_t* hw;  // [a->batch][2] latent (H_b, W_b), host
    long long elems;    // length of the flat state
    int n_max;          // longest sequence
};
// validates a size list against the engine and the step arguments (refusals by name), fills `pc` and stores the device table on stream s
// (engine.hip)
int packed_call_begin(lt_engine* e, const char* who, const int32_t* hw_host, const lt_step_args* a, int use_cfg, PackedCall* pc, hipStream_t s);
// What one evaluation is: its kind (eval_kind.h: one line per kind, and what follows from it), and
// pc - a packed batch: x_in / out are its flat state (LT_KIND_WHOLE only);
// cfg_dev - the kinds that read their guidance scale from device memory: one float, staged into e->g_cfg, which the closing kernel reads, so
// the scale is no part of the graph key; cfg_dev == e->g_cfg: the scale is in place.  (LT_KIND_COND_ONLY stages nothing.)
struct EvalSpec {
    LtEvalKind kind = LT_KIND_WHOLE;
    const PackedCall* pc = nullptr;
    const float* cfg_dev = nullptr;
};
// one model evaluation [+ CFG combine], through a cached HIP graph where that pays (engine.hip).  The caller has allocated what the kind keeps
// (ensure_delta, ensure_skip_buf, ensure_step_cache), has put the rule's parameters / the skip-layer scale in place, and answers for a stored
// difference or residual being there; a part behind a step-caching head follows a head of the same step arguments with no other evaluation
// between (e->cache_head; refused by name otherwise)
int forward_graphed(lt_engine* e, const void* x_in, const float* t_dev, void* out, const lt_step_args* a, int use_cfg, hipStream_t s,
                    const EvalSpec& spec = {});
// the buffers of step caching: allocated on the first call, before anything is launched (engine.hip)
int ensure_step_cache(lt_engine* e);
// the difference buffer of guidance reuse: allocated on the first call, before anything is launched (engine.hip)
int ensure_delta(lt_engine* e);
// ... and the skip buffer of skip-layer guidance (engine.hip)
int ensure_skip_buf(lt_engine* e);
// ... and the buffers of projected guidance (engine.hip)
int ensure_project(lt_engine* e);
// The rule form of one call's LT_KIND_RULE evaluations: set for the scope, 0 again behind it
struct ProjectScope {
    lt_engine* e;
    ProjectScope(lt_engine* eng, int form) : e(eng) { e->rule_form = form; }
    ProjectScope(const ProjectScope&) = delete;
    ProjectScope& operator=(const ProjectScope&) = delete;
    ~ProjectScope() { e->rule_form = 0; }
};
// The layer sets of one call: the blocks left out and the blocks whose self-attention is perturbed.  set() refuses by
// name - an index outside 0 .. L-1, a repeated index, more indices than L, a skip set that leaves no layer, an index in both sets - and
// otherwise stores each set in ascending order; the destructor empties both, so no entry point returns with a set left behind
struct SkipScope {
    lt_engine* e;
    explicit SkipScope(lt_engine* eng) : e(eng) {}
    SkipScope(const SkipScope&) = delete;
    SkipScope& operator=(const SkipScope&) = delete;
    ~SkipScope() { e->skip.clear(); e->perturb.clear(); e->blur.clear(); }
    int set(const char* who, const int32_t* skip_host, int n_skip, const int32_t* perturb_host = nullptr, int n_perturb = 0);
    // the skip set and the set of blurred blocks (the perturb set stays empty); the call has run ensure_blur for its sigma
    int set_blur(const char* who, const int32_t* skip_host, int n_skip, const int32_t* blur_host, int n_blur);
};
// the refusals of SkipScope::set_blur alone (nothing stored): both sets, that they are disjoint, and sigma
int check_blur_sets(const lt_engine* e, const char* who, const int32_t* skip_host, int n_skip, const int32_t* blur_host, int n_blur, float sigma);
// ... and of the call's grid: the radius sigma stands for must be reflectable on latent_h / patch x latent_w / patch image tokens (n_blur 0: nothing)
int check_blur_radius(const lt_engine* e, const char* who, const lt_step_args* a, int n_blur, float sigma);
// smoothed-energy guidance: the blurred-query buffer and the tap words, allocated on the first call, before anything is launched; then the taps
// of this call's sigma put in place on stream s (one synchronisation: they come from pageable memory) and mode / radius stored (engine.hip)
int ensure_blur(lt_engine* e, float sigma, hipStream_t s);
// the refusals of SkipScope::set alone (nothing stored): both sets, and that they are disjoint
int check_layer_sets(const lt_engine* e, const char* who, const int32_t* skip_host, int n_skip, const int32_t* perturb_host, int n_perturb);
// ... of a call that takes a skip set only
int check_skip_set(const lt_engine* e, const char* who, const int32_t* skip_host, int n_skip);
// true while stream s records into a graph (the caller's torch.cuda.graph / hipStreamBeginCapture, or the engine's own cache)
bool stream_capturing(hipStream_t s);
// the entry points that allocate, synchronise or copy from host memory cannot be recorded into a caller's graph: non-zero after
// lt_set_error("<who>: ... capture ...") when s is capturing - called before anything is launched, so the capture stays valid (engine.hip)
int refuse_if_capturing(hipStream_t s, const char* who);
// ... and while lt_profile_enable is on, the calls that are otherwise recordable (a model evaluation, lt_prepare_prompt / _labels): the
// profile brackets launches with HIP events.  Costs no stream query while the profile is off (engine.hip)
int refuse_profile_if_capturing(const lt_engine* e, hipStream_t s, const char* who);
// the softmax scale of an evaluation of N tokens under the engine's rule (model.py:373-376, visual_anagrams/models/nextdit.py:331-335), and the
// refusal of a shape the anagram fork's query chunks do not cover; non-zero after lt_set_error (engine.hip)
int softmax_scale_for(const lt_engine* e, const lt_step_args* a, int N, float* scale);
// frees the tables of lt_set_views (samplers.hip)
void drop_views(lt_engine* e);
// frees the buffers of lt_set_windows (samplers.hip)
void drop_windows(lt_engine* e);
