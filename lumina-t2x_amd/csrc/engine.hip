// Host side of the C ABI (include/lumina_dit.h): engine object, weight arena, workspace, prompt preparation and ONE model evaluation - the
// per-NFE launch sequence of NextDiT.forward / forward_with_cfg (lumina_next_t2i/models/model.py:836-913) and its HIP-graph cache - plus
// the MoE routing, profiling and option hooks.  The whole-trajectory samplers (lt_sample_*) are in samplers.hip, the operator-level
// entry points (lt_op_*) in ops_abi.hip, which needs no engine state; engine.h holds what this file and samplers.hip share.
//
// Everything here is asynchronous on the caller's stream: no host<->device sync inside a step (the
// reference syncs >= 25 times per NFE: t[0].item() model.py:888, nonzero/.item() per layer :288-289).
// Step-invariant work is hoisted: text K/V of all layers and the caption embedding are computed once per
// prompt (lt_prepare_prompt); the adaLN vectors of all layers are one GEMV per NFE; the RoPE table is
// a 2 x 384 x hd/4 (cos,sin) table rebuilt only when scale_factor changes.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "engine.h"
#include "kernels.h"

// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
void lt_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* lt_last_error(void) { return g_err; }
extern "C" const char* lt_version(void) { return "lumina_dit gfx950 r5"; }

namespace {

constexpr float LOG2E = 1.44269504088896340736f;
// Kernel-selection options (options.h; lt_set_option = process default, lt_engine_set_option = per-engine override): those that pick a transformer
// block's launches are described at the routes they pick (QkvRoute, PostRoute, BlockPlan below).  graph: 1 = a model evaluation (~250 launches) is
// captured into a HIP graph per (arguments, shapes) and replayed; 2 (default) = above 1024 rows only (forward_graphed).  Every option change moves
// lt_opt_generation(), which is part of the graph key (kernel selection is baked into a captured graph).

VariantDesc variant_desc(int variant) {
    VariantDesc v{};
    if (variant == LT_VARIANT_NEXT_T2I) {
        v = {4, {-1, -1}, {0, 2}, {1, 3}, true, true, true, true, false, false, false, 1};
    } else if (variant == LT_VARIANT_NEXT_IMAGENET || variant == LT_VARIANT_NEXT_MOE_TIME || variant == LT_VARIANT_NEXT_MOE_SPACE) {
        // (the single-MoE models of Next-DiT-MoE/models/models.py / models1.py are the ImageNet block with its FFN replaced
        //  by one MoeLayer: four adaLN chunks, same norms - models.py:749-758)
        v = {4, {-1, -1}, {0, 2}, {1, 3}, false, true, true, false, true, false, false, 2};
    } else if (variant == LT_VARIANT_NEXT_MOE) {
        // models2.py:783-784: scale_msa, gate_msa, scale_mlp_time, gate_mlp_time, scale_mlp_space, gate_mlp_space;
        // index [1] is the time branch, the space branch uses chunks 4 / 5 (run_forward)
        v = {6, {-1, -1}, {0, 2}, {1, 3}, false, true, true, false, true, false, false, 2};
    } else {  // LT_VARIANT_FLAG_T2I
        v = {6, {0, 3}, {1, 4}, {2, 5}, true, false, false, true, false, true, true, 2};
    }
    return v;
}

int dev_alloc(lt_engine* e, void** out, size_t bytes, bool zero = true) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    LT_CHECK_HIP(hipMalloc(&p, bytes));
    if (zero) LT_CHECK_HIP(hipMemset(p, 0, bytes));
    e->allocs.push_back({p, bytes});
    *out = p;
    return 0;
}
struct ProfScope {
    lt_engine* e;
    int k;
    hipStream_t s;
    bool on = false, attach = false;  // attach: the launch carries the event pair itself (no records here)
    size_t slot = 0;
    hipEvent_t ev0() const { return on ? e->prof[k].ev[slot].first : nullptr; }
    hipEvent_t ev1() const { return on ? e->prof[k].ev[slot].second : nullptr; }
    ProfScope(lt_engine* e_, int klass, double flops, hipStream_t s_, bool attach_ = false) : e(e_), k(klass), s(s_), attach(attach_) {
        if (e->tally) {  // graph capture: no events inside a graph, only the bookkeeping a replay will add
            e->tally->flops[k] += flops;
            e->tally->launches[k] += 1;
            return;
        }
        if (!e->prof_on || !((e->prof_mask >> k) & 1)) return;
        ProfClass& pc = e->prof[k];
        pc.flops += flops;
        pc.launches += 1;
        if (pc.launches > pc.skip && pc.used < pc.ev.size() && pc.used < pc.budget) {
            on = true;
            slot = pc.used++;
            if (!attach) (void)hipEventRecord(pc.ev[slot].first, s);
        }
    }
    ~ProfScope() {
        if (on && !attach) (void)hipEventRecord(e->prof[k].ev[slot].second, s);
    }
};

// "gemm_prefetch" 3: the weight panels of the next 512-row-class GEMM are read by rider workgroups inside the row kernel that precedes it.
// (Option 2 - the same reads on a side stream beside the preceding kernel - lost 33 % to +37 us per layer of cross-stream dependencies
//  and was removed in round 5 together with its fork / join state)
void prefetch_rider(lt_engine* e, PrefetchRider* r, const u16* A, int lda, const u16* W, int ldw, u16* C, int ldc, int M, int N, int K, int epi) {
    if (lt_opt(OPT_GEMM_PREFETCH) != 3 || M > 1024) return;
    GemmArgs g;
    g.A = A; g.W = W; g.C = C; g.bias = nullptr; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldc = ldc;
    g.bias_dtype = -1;
    g.splitk_part = e->splitk_part; g.splitk_cnt = e->splitk_cnt; g.splitk_tiles = e->splitk_tiles;
    if (!gemm_prefetch_rider(g, epi, r)) *r = PrefetchRider();
}

// one GEMM launch in the profile's class 0; the dispatch packet carries the event pair itself
int profiled_gemm(lt_engine* e, const GemmArgs& g, int epi, double flops, hipStream_t s, int variant = 0) {
    ProfScope ps(e, 0, flops, s, true);
    return launch_gemm_bf16(g, epi, variant, s, ps.ev0(), ps.ev1());
}

// ystat_slots (optional, out): > 0 when the launch left the rows' sum-of-squares partials in e->ystat (option grn_ystat; GemmArgs::ystat)
int gemm(lt_engine* e, const u16* A, int lda, const u16* W, int ldw, u16* C, int ldc, int M, int N, int K,
         const u16* bias, int epi, hipStream_t s, int* ystat_slots = nullptr, int pair_ab = 0, int pair_c = 0, int variant = 0) {
    GemmArgs g;
    g.A = A; g.W = W; g.C = C; g.bias = bias; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldc = ldc;
    g.bias_dtype = bias ? 1 : -1;
    g.pair_ab = pair_ab; g.pair_c = pair_c;
    g.splitk_part = e->splitk_part; g.splitk_cnt = e->splitk_cnt; g.splitk_tiles = e->splitk_tiles;  // (the launcher decides)
    if (ystat_slots) {
        *ystat_slots = 0;
        const int ys = lt_opt(OPT_GRN_YSTAT) && !bias ? gemm_ystat_slots(g, epi) : 0;
        if (ys > 0 && ys <= e->ystat_cap) { g.ystat = e->ystat; g.ystat_slots = ys; *ystat_slots = ys; }
    }
    if (lt_opt(OPT_GEMM_PREFETCH) == 1 && M <= 1024 && launch_gemm_prefetch_w(g, epi, s)) return 1;
    return profiled_gemm(e, g, epi, 2.0 * M * (double)N * K, s, variant);
}

int attention(lt_engine* e, const AttnArgs& a, hipStream_t s) {
    ProfScope ps(e, 1, 4.0 * a.B * a.H * (double)a.N * (a.Nk + (a.tk ? a.Tk : 0)) * a.hd, s);
    return launch_attention(a, s);
}

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ---- weight table -----------------------------------------------------------------------------------
struct Slot {
    u16* dst;
    int rows, cols, dst_ld, r0, row_map;
};

bool parse_layer_key(const char* key, int* layer, std::string* rest) {
    if (strncmp(key, "layers.", 7) != 0) return false;
    char* end = nullptr;
    long l = strtol(key + 7, &end, 10);
    if (end == key + 7 || *end != '.') return false;
    *layer = (int)l;
    *rest = std::string(end + 1);
    return true;
}

int find_slot(lt_engine* e, const std::string& key, Slot* s) {
    const int d = e->d, A = e->A, cap = e->cap, F = e->F, dkv = e->dkv;
    int l;
    std::string r;
    auto set = [&](u16* dst, int rows, int cols, int ld, int r0 = 0, int map = 0) {
        s->dst = dst; s->rows = rows; s->cols = cols; s->dst_ld = ld; s->r0 = r0; s->row_map = map;
        return 0;
    };
    if (parse_layer_key(key.c_str(), &l, &r)) {
        LT_REQUIRE(l >= 0 && l < e->L, "weight key %s: layer out of range", key.c_str());
        LayerW& w = e->lw[l];
        const int cd = e->chunks * d;
        if (r == "attention.wq.weight") return set(w.wqkv, d, d, d, 0);
        if (r == "attention.wk.weight") return set(w.wqkv, dkv, d, d, d);
        if (r == "attention.wv.weight") return set(w.wqkv, dkv, d, d, d + dkv);
        if (r == "attention.wo.weight") return set(w.wo, d, d, d);
        if (r == "attention.wk_y.weight") return set(w.wkvy, dkv, cap, cap, 0);
        if (r == "attention.wv_y.weight") return set(w.wkvy, dkv, cap, cap, dkv);
        if (r == "attention.q_norm.weight") return set(w.q_norm_w, 1, d, d);
        if (r == "attention.q_norm.bias") return set(w.q_norm_b, 1, d, d);
        if (r == "attention.k_norm.weight") return set(w.k_norm_w, 1, dkv, dkv);
        if (r == "attention.k_norm.bias") return set(w.k_norm_b, 1, dkv, dkv);
        if (r == "attention.ky_norm.weight") return set(w.ky_norm_w, 1, dkv, dkv);
        if (r == "attention.ky_norm.bias") return set(w.ky_norm_b, 1, dkv, dkv);
        if (r == "attention.gate") return set(w.gate, 1, e->H, e->H);
        if (e->E == 0) {
            if (r == "feed_forward.w1.weight") return set(w.w13, F, d, d, 0, 1);
            if (r == "feed_forward.w3.weight") return set(w.w13, F, d, d, 0, 2);
            if (r == "feed_forward.w2.weight") return set(w.w2, d, F, F);
        }
        if (e->E > 0 && e->moe_mode != 0) {  // one MoeLayer as `feed_forward` (models.py:700-707 / models1.py:700-707)
            const bool time = e->moe_mode == 1;
            if (r == "attention_norm.weight") return set(w.attn_norm2, 1, d, d);
            if (r == "ffn_norm.weight") return set(w.ffn_norm2, 1, d, d);
            if (r == "feed_forward.gate.weight") return time ? set(w.gate_t, e->E, A, A) : set(w.gate_s, e->E, d, d);
            const char* pre = "feed_forward.experts.";
            const size_t pl = strlen(pre);
            if (r.compare(0, pl, pre) == 0) {
                char* end = nullptr;
                const long ex = strtol(r.c_str() + pl, &end, 10);
                LT_REQUIRE(end != r.c_str() + pl && ex >= 0 && ex < e->E, "weight key %s: expert out of range", key.c_str());
                const std::string tail(end);
                u16* w13 = (time ? w.w13_t : w.w13_s) + (size_t)ex * 2 * F * d;
                u16* w2 = (time ? w.w2_t : w.w2_s) + (size_t)ex * d * F;
                if (tail == ".w1.weight") return set(w13, F, d, d, 0, 1);
                if (tail == ".w3.weight") return set(w13, F, d, d, 0, 2);
                if (tail == ".w2.weight") return set(w2, d, F, F);
            }
        } else if (e->cfg.variant == LT_VARIANT_NEXT_MOE) {
            if (r == "attention_norm.weight") return set(w.attn_norm2, 1, d, d);
            if (r == "ffn_norm_time.weight") return set(w.norm_time, 1, d, d);
            if (r == "ffn_norm_space.weight") return set(w.norm_space, 1, d, d);
            if (r == "feed_forward_time.gate.weight") return set(w.gate_t, e->E, A, A);
            if (r == "feed_forward_space.gate.weight") return set(w.gate_s, e->E, d, d);
            for (int br = 0; br < 2; ++br) {
                const char* pre = br == 0 ? "feed_forward_time.experts." : "feed_forward_space.experts.";
                const size_t pl = strlen(pre);
                if (r.compare(0, pl, pre) != 0) continue;
                char* end = nullptr;
                const long ex = strtol(r.c_str() + pl, &end, 10);
                LT_REQUIRE(end != r.c_str() + pl && ex >= 0 && ex < e->E, "weight key %s: expert out of range", key.c_str());
                const std::string tail(end);
                u16* w13 = (br == 0 ? w.w13_t : w.w13_s) + (size_t)ex * 2 * F * d;
                u16* w2 = (br == 0 ? w.w2_t : w.w2_s) + (size_t)ex * d * F;
                if (tail == ".w1.weight") return set(w13, F, d, d, 0, 1);
                if (tail == ".w3.weight") return set(w13, F, d, d, 0, 2);
                if (tail == ".w2.weight") return set(w2, d, F, F);
            }
        } else if (e->cfg.variant == LT_VARIANT_NEXT_T2I) {
            if (r == "attention_norm1.weight") return set(w.attn_norm1, 1, d, d);
            if (r == "attention_norm2.weight") return set(w.attn_norm2, 1, d, d);
            if (r == "ffn_norm1.weight") return set(w.ffn_norm1, 1, d, d);
            if (r == "ffn_norm2.weight") return set(w.ffn_norm2, 1, d, d);
        } else if (e->cfg.variant == LT_VARIANT_NEXT_IMAGENET) {  // post-norms carry the weight (models.py:735-738)
            if (r == "attention_norm.weight") return set(w.attn_norm2, 1, d, d);
            if (r == "ffn_norm.weight") return set(w.ffn_norm2, 1, d, d);
        } else {  // Flag-DiT: pre-norms only (lumina_t2i model.py:556-557)
            if (r == "attention_norm.weight") return set(w.attn_norm1, 1, d, d);
            if (r == "ffn_norm.weight") return set(w.ffn_norm1, 1, d, d);
        }
        if (r == "attention_y_norm.weight") return set(w.y_norm, 1, cap, cap);
        if (r == "adaLN_modulation.1.weight") return set(e->adaln_w, cd, A, A, l * cd);
        if (r == "adaLN_modulation.1.bias") return set(e->adaln_b + (size_t)l * cd, 1, cd, cd);
    } else {
        const int cd = e->chunks * d;
        if (key == "x_embedder.weight") return set(e->xemb_w, d, e->cfg.in_channels * e->cfg.patch_size * e->cfg.patch_size, e->kpad);
        if (key == "x_embedder.bias") return set(e->xemb_b, 1, d, d);
        if (key == "t_embedder.mlp.0.weight") return set(e->t0_w, A, 256, 256);
        if (key == "t_embedder.mlp.0.bias") return set(e->t0_b, 1, A, A);
        if (key == "t_embedder.mlp.2.weight") return set(e->t2_w, A, A, A);
        if (key == "t_embedder.mlp.2.bias") return set(e->t2_b, 1, A, A);
        if (key == "cap_embedder.0.weight") return set(e->capln_w, 1, cap, cap);
        if (key == "cap_embedder.0.bias") return set(e->capln_b, 1, cap, cap);
        if (key == "cap_embedder.1.weight") return set(e->cape_w, A, cap, cap);
        if (key == "cap_embedder.1.bias") return set(e->cape_b, 1, A, A);
        if (key == "pad_token") return set(e->pad_token, 1, d, d);
        if (key == "eol_token" && e->v.eol) return set(e->eol_token, 1, d, d);
        if (key == "y_embedder.embedding_table.weight" && e->v.labels) return set(e->label_table, e->label_rows, A, A);
        const int fd = e->v.final_chunks * d;
        if (key == "final_layer.linear.weight") return set(e->final_w, e->nfinal, d, d);
        if (key == "final_layer.linear.bias") return set(e->final_b, 1, e->nfinal, e->nfinal);
        if (key == "final_layer.adaLN_modulation.1.weight") return set(e->adaln_w, fd, A, A, e->L * cd);
        if (key == "final_layer.adaLN_modulation.1.bias") return set(e->adaln_b + (size_t)e->L * cd, 1, fd, fd);
    }
    lt_set_error("unknown weight key '%s' for this variant", key.c_str());
    return 2;
}

// (cos,sin) factor table(s) for this call's RoPE arguments; rebuilt only when they change - or always once a caller has recorded an
// evaluation into a graph of its own (layout_pinned): that graph rebuilds the table for ITS arguments on every replay, which the host
// does not see, and a rebuild recorded during the capture has not run at all
int ensure_rope(lt_engine* e, const lt_step_args* a, hipStream_t s) {
    const float ntk = a->ntk_factor > 0.f ? a->ntk_factor : 1.0f;
    const float sf = a->scale_factor > 0.f ? a->scale_factor : 1.0f;
    if (!e->layout_pinned && e->rope_scale == sf && e->rope_ntk == ntk) return 0;
    if (e->cfg.variant == LT_VARIANT_NEXT_T2I) {
        if (launch_rope_table_2d(e->rope, e->rope_len, e->hd, 10000.0f, sf, s, e->rope_tr)) return 1;
    } else {
        // both branches identical: theta * ntk_factor, positions / rope_scaling_factor (models.py:1001-1005, model.py:948-955)
        const int step = e->v.rope_1d ? 2 : 4;
        if (launch_rope_table(e->rope, e->rope_len, e->hd, step, 10000.0f * ntk, sf, 10000.0f * ntk, sf, 1, s, e->rope_tr)) return 1;
    }
    e->rope_scale = sf;
    e->rope_ntk = ntk;
    return 0;
}

// tile bound of THIS call's row count, not of the engine's capacity: a capacity-sized launch would be mostly padding tiles, and the XCD-contiguous
// tile order would put every real tile on XCD 0 (measured: 255 us instead of 60 us per expert GEMM at 512 rows in an engine sized for 8192)
int moe_tiles_for(const lt_engine* e, int M) { return (int)((2 * (size_t)M + (size_t)e->E * 255 + 255) / 256); }
// the two grouped GEMMs of a MoE feed-forward of M rows, as launched and as plan_block asks the dispatch about them: SwiGLU on the un-sorted
// FFN input e->h (the GEMM gathers its rows through the plan's inverse map `src`, no expert-sorted copy), then W2
void moe_gemm_args(const lt_engine* e, const u16* w13, const u16* w2, const int* tile_expert, const int* src, int M, GemmArgs& g13, GemmArgs& g2) {
    const int d = e->d, F = e->F;
    g13 = GemmArgs{};
    g13.bias_dtype = -1; g13.tile_expert = tile_expert; g13.M = moe_tiles_for(e, M) * 256;
    g2 = g13;
    g13.A = e->h; g13.a_row_map = src; g13.a_map_rows = M; g13.W = w13; g13.C = e->moe_us; g13.N = 2 * F; g13.K = d; g13.lda = d; g13.ldw = d; g13.ldc = F;
    g13.w_expert_stride = (long long)2 * F * d;
    g2.A = e->moe_us; g2.W = w2; g2.C = e->moe_ys; g2.N = d; g2.K = F; g2.lda = F; g2.ldw = F; g2.ldc = d; g2.w_expert_stride = (long long)d * F;
}

// one MoE feed-forward (branch 0 = TimeMoeLayer on the timestep embedding, 1 = SpaceMoeLayer on the tokens;
// models2.py:451-506): e->h -> e->o
// routed: sel / wts of this (token-routed) branch were already written by the row kernel that produced its input (GatedResArgs::route_*)
// pair: the experts' weights are in the pair layout (run_forward decided; ensure_weight_layout), and so is the SwiGLU output e->moe_us
int moe_ffn(lt_engine* e, LayerW& w, int layer, int branch, int M, int N, int B, hipStream_t s, bool routed = false, bool pair = false) {
    const int d = e->d, F = e->F;
    MoeArgs m;
    m.x = e->h; m.rows = M; m.rows_per_sample = N; m.d = d; m.E = e->E;
    const bool hoisted = branch == 0 && e->moe_tp_live;  // this layer's time plan was written at the top of the evaluation (run_forward)
    m.sel = e->moe_sel; m.wts = e->moe_wts; m.pos = e->moe_pos; m.tile_expert = e->moe_tile_expert; m.max_tiles = moe_tiles_for(e, M);
    m.src = e->moe_src;
    if (hoisted) {
        m.sel = e->moe_tp_sel + (size_t)layer * e->moe_tp_stride_rows; m.pos = e->moe_tp_pos + (size_t)layer * e->moe_tp_stride_rows;
        m.wts = e->moe_tp_wts + (size_t)layer * e->moe_tp_stride_rows; m.src = e->moe_tp_src + (size_t)layer * e->moe_tp_stride_src;
        m.tile_expert = e->moe_tp_tile_expert + (size_t)layer * e->moe_tiles;
    }
    m.gate_w = nullptr; m.sample_logits = nullptr; m.forced = nullptr;
    {
        ProfScope ps(e, 2, 0, s);
        if (branch == 0) {  // gate(cond) with cond = t_embedder(t) (models2.py:462, :950-951): computed for all layers at once, run_forward
            m.sample_logits = e->moe_logits + (size_t)layer * e->E;
            m.sample_ld = e->L * e->E;
        } else {
            m.gate_w = w.gate_s;
        }
        const size_t slot = ((size_t)layer * 2 + branch) * (size_t)e->cfg.max_batch * e->cfg.max_tokens * 2;
        if (e->moe_force_rows) {
            LT_REQUIRE(e->moe_force_rows == M, "forced MoE routing was given for %d rows, this call has %d", e->moe_force_rows, M);
            m.forced = e->moe_force + slot;
        }
        if (branch != 0 && !routed && launch_moe_route(m, s)) return 1;  // (the time branch routes inside the plan kernel)
        if (!hoisted && launch_moe_plan(m, s)) return 1;
        if (e->moe_rec_on) {
            LT_CHECK_HIP(hipMemcpyAsync(e->moe_rec + slot, m.sel, (size_t)M * 2 * sizeof(int), hipMemcpyDeviceToDevice, s));
            e->moe_rec_rows = M;
        }
    }
    // grouped SwiGLU GEMM: each 256-row tile multiplies with its expert's packed w1|w3 - then the experts' W2
    GemmArgs g13, g2;
    moe_gemm_args(e, branch == 0 ? w.w13_t : w.w13_s, branch == 0 ? w.w2_t : w.w2_s, m.tile_expert, m.src, M, g13, g2);
    g13.pair_ab = pair ? 2 : 0; g13.pair_c = pair;  // (A is gathered row by row from e->h: row-major)
    if (profiled_gemm(e, g13, 1, 2.0 * (2.0 * M) * (2.0 * F) * d, s)) return 1;  // algorithmic: every token visits two experts
    if (lt_opt(OPT_GEMM_TAIL_SPLIT) && e->tail_part) { g2.tail_part = e->tail_part; g2.tail_cnt = e->tail_cnt; g2.tail_cap_parts = e->tail_cap_parts; g2.tail_max_parts = lt_opt(OPT_GEMM_TAIL_SPLIT) == 2 ? 2 : 4; }
    g2.pair_ab = pair ? 3 : 0;
    if (profiled_gemm(e, g2, 0, 2.0 * (2.0 * M) * (double)d * F, s)) return 1;
    // (the top-2 combine of e->moe_ys is formed by the gated_residual_norm launch that consumes this branch: moe_y() below)
    return 0;
}

// the branch output of a MoE FFN as gated_residual_norm takes it: experts' outputs + routing, combined on the way in
// layer >= 0: the branch is the time router's and its plan may be the hoisted one of that layer
void moe_y(const lt_engine* e, GatedResArgs& g, int time_layer = -1) {
    g.y = nullptr; g.moe_ys = e->moe_ys; g.moe_pos = e->moe_pos; g.moe_wts = e->moe_wts;
    if (time_layer >= 0 && e->moe_tp_live) {
        g.moe_pos = e->moe_tp_pos + (size_t)time_layer * e->moe_tp_stride_rows;
        g.moe_wts = e->moe_tp_wts + (size_t)time_layer * e->moe_tp_stride_rows;
    }
}

// one forward pass of the configured family [+ CFG combine]:
//   NextDiT.forward / forward_with_cfg   lumina_next_t2i/models/model.py:836-913
//   DiT_Llama (ImageNet)                 Next-DiT-ImageNet/models/models.py:920-974
//   DiT_Llama (Flag-DiT)                 lumina_t2i/models/model.py:829-922
//
// Packed variable-resolution batch (NextDiT.patchify_and_embed list branch, model.py:789-834): sample b is its own
// [C, H_b, W_b] tensor; sequences are padded to the longest one with `pad_token`, padded positions rotate like the sample's
// last token, are masked as KEYS (x_mask, :407-415) and dropped again by unpatchify (:757-768).  Only the plain forward of
// the text-conditional Next-DiT has this path in the reference.
struct PackedDesc {
    const void* const* x_ptrs;  // [B] device pointers
    void* const* out_ptrs;      // [B] device pointers, each [in_channels, H_b, W_b]
    const int32_t* hw;          // [B][2] latent (H_b, W_b), host
    // the flat form (lt_forward_cfg_packed / lt_sample_ode_packed; x_ptrs / out_ptrs null): one state buffer, the ragged kernels of packed.hip
    const void* x_flat = nullptr;
    void* out_flat = nullptr;
    const int* tab = nullptr;   // device PackedTable (kernels.h) of the same size list
};

// all four GEMM weights of every dense block -> the row-pair-interleaved layout (want) or back to row-major, in place, on stream s.
// recording: s is the caller's capturing stream (want is false there).  These launches run at every replay of the caller's graph and not now,
// so they are conditional on the device word e->w_pair_dev (whoever comes first converts, everyone after finds 0 and does nothing), and the
// next eager call owes the same conditional conversion (w_owed) before its own kernels read the weights.
int ensure_weight_layout(lt_engine* e, bool want, hipStream_t s, bool recording = false) {
    if (e->w_pair == want && !e->w_owed) return 0;
    LT_REQUIRE(!want || (!e->layout_pinned && !recording), "pair layout: the weights are pinned row-major (a caller's graph holds row-major kernels)");
    const int* only_if = recording || e->w_owed ? e->w_pair_dev : nullptr;
    for (int l = 0; l < e->L; ++l) {
        LayerW& w = e->lw[l];
        if (e->E == 0) {
            if (launch_pair_layout(w.wqkv, e->qkvn, e->d, want, s, only_if)) return 1;
            if (launch_pair_layout(w.wo, e->d, e->d, want, s, only_if)) return 1;
            if (launch_pair_layout(w.w13, 2LL * e->F, e->d, want, s, only_if)) return 1;
            if (launch_pair_layout(w.w2, e->d, e->F, want, s, only_if)) return 1;
        } else {  // MoE families: the experts' weights only ([E][2 F][d] / [E][d][F]: an expert's rows are an even count, pairs stay inside it)
            for (u16* w13 : {w.w13_t, w.w13_s}) if (w13 && launch_pair_layout(w13, 2LL * e->E * e->F, e->d, want, s, only_if)) return 1;
            for (u16* w2 : {w.w2_t, w.w2_s}) if (w2 && launch_pair_layout(w2, (long long)e->E * e->d, e->F, want, s, only_if)) return 1;
        }
    }
    LT_CHECK_HIP(hipMemsetAsync(e->w_pair_dev, want ? 1 : 0, sizeof(int), s));  // (behind the last conversion, in stream order)
    e->w_pair = want;
    e->w_owed = recording;
    ++e->layout_flips_total;
    return 0;
}

// ---- one model evaluation: run_forward and its stages.  They share Dims, the shapes of the call, and BlockPlan (below), the launch route of a
// transformer block: neither depends on the layer - shapes, family, prompt state and the option snapshot (LtOptScope) are constant for the call
struct Dims {
    int B, N, Npad, M, Hp, Wp, Wrow;  // M = B x N rows; a packed batch: N / Hp / Wp of its longest sample.  Wrow: tokens per latent row
    float sm_scale;
    // packed batches: per-sample token count / grid width for the rotary positions and the key mask, on the host and on the device (null: a
    // tensor state); nk_dev: the key counts the self-attention masks by (null also in the flat form when every sample has the longest length)
    int ntok[64], gw[64];
    const int *ntok_dev = nullptr, *gw_dev = nullptr, *nk_dev = nullptr;
    bool pk_full = true;  // no sample is shorter than the longest one: no padded keys to mask
};
const u16* mod_chunk(const lt_engine* e, int layer, int idx) { return idx < 0 ? nullptr : e->mod + ((size_t)layer * e->chunks + idx) * e->d; }
// the final layer's modulation, behind the L layers' chunks: [shift,] scale (model.py:657-661 / models.py:829-832)
const u16* final_shift(const lt_engine* e) { return e->v.final_chunks == 2 ? mod_chunk(e, e->L, 0) : nullptr; }
const u16* final_scale(const lt_engine* e) { return mod_chunk(e, e->L, 0) + (e->v.final_chunks == 2 ? e->d : 0); }
int cfg_channels(const lt_step_args* a) { return a->cfg_channels > 0 ? a->cfg_channels : 3; }
// what every closing step of a branch shares: x += gate' * post(y); h = the next pre-norm of x, modulated
GatedResArgs gated_res_args(const lt_engine* e, const Dims& dm) {
    GatedResArgs g{};
    g.x = e->x; g.h = e->h; g.rows = dm.M; g.rows_per_batch = dm.N; g.d = e->d; g.ld_mod = e->ld_mod;
    g.eps = e->cfg.norm_eps; g.eps_next = 1e-6f; g.scale_pre = 1;
    return g;
}

// The closing step of an evaluation on a tensor state: frows -> `out` in the caller's layout, guided as the kind says.  The kinds that read
// their scale from device memory find it in e->g_cfg[0], the rule's blend and limit in [1..2], the skip-layer scale in [3]; a half-row kind
// ran B rows and writes 2 B (the kernels count output rows)
int close_forward(lt_engine* e, void* out, const lt_step_args* a, int use_cfg, int B, int Wrow, LtEvalKind kind, hipStream_t s) {
    const lt_config& c = e->cfg;
    const int p = c.patch_size, Bout = lt_eval_traits(kind).half ? 2 * B : B;
    const int cfg_ch = cfg_channels(a);
    const int guided_ch = cfg_ch < c.in_channels ? cfg_ch : c.in_channels;  // (the channels the closing kernel guides)
    const float* g = e->g_cfg;
    switch (kind) {
    case LT_KIND_WHOLE: case LT_KIND_CACHE_BLOCKS: case LT_KIND_CACHE_APPLY:
        return launch_unpatchify_cfg(e->frows, e->nfinal, out, a->io_dtype, B, c.in_channels, c.out_channels, a->latent_h, a->latent_w, p, use_cfg,
                                     a->cfg_scale, cfg_ch, Wrow, s);
    case LT_KIND_DEV_GUIDED: case LT_KIND_COND_ONLY:
        return launch_unpatchify_cfg_dev(e->frows, e->nfinal, out, a->io_dtype, Bout, c.in_channels, c.out_channels, a->latent_h, a->latent_w, p,
                                         use_cfg, g, cfg_ch, Wrow, kind == LT_KIND_COND_ONLY ? 1 : 0, s);
    case LT_KIND_RULE:  // guidance_stats, then the kernel that multiplies by the per-sample factor - or the two kernels of a projected form
        if (e->rule_form != 0) {  // (the scale in g[0] as ever, eta / beta / r in e->p_par[1..3], APG's momentum advanced in place)
            if (launch_guidance_project_stats(e->frows, e->nfinal, B, c.out_channels, a->latent_h, a->latent_w, p, guided_ch, Wrow, e->rule_form,
                                              e->p_par, e->p_mom, e->p_stats, s)) return 1;
            return launch_unpatchify_cfg_project(e->frows, e->nfinal, out, a->io_dtype, B, c.in_channels, c.out_channels, a->latent_h, a->latent_w,
                                                 p, use_cfg, g, guided_ch, Wrow, 0, e->rule_form, e->p_stats, e->p_par, e->p_mom, nullptr, s);
        }
        if (launch_guidance_stats(e->frows, e->nfinal, B, c.out_channels, a->latent_h, a->latent_w, p, g, guided_ch, Wrow, e->g_stats, s)) return 1;
        return launch_unpatchify_cfg_rule(e->frows, e->nfinal, out, a->io_dtype, B, c.in_channels, c.out_channels, a->latent_h, a->latent_w, p,
                                          use_cfg, g, guided_ch, Wrow, 0, e->g_stats, g + 1, g + 2, nullptr, s);
    case LT_KIND_REUSE_STORE: case LT_KIND_REUSE_AGAIN:
        return launch_unpatchify_cfg_reuse(e->frows, e->nfinal, out, a->io_dtype, Bout, c.in_channels, c.out_channels, a->latent_h, a->latent_w, p,
                                           g, guided_ch, Wrow, e->g_delta, kind == LT_KIND_REUSE_AGAIN ? 1 : 0, s);
    case LT_KIND_SLG_STORE: case LT_KIND_SLG_GUIDED: case LT_KIND_SLG_COND:
        return launch_unpatchify_cfg_slg(e->frows, e->nfinal, out, a->io_dtype, Bout, c.in_channels, c.out_channels, a->latent_h, a->latent_w, p,
                                         g, g + 3, guided_ch, Wrow, e->g_skip, lt_slg_kernel_mode(kind), s);
    case LT_KIND_CACHE_HEAD: case LT_KIND_COUNT: break;  // (a head returns before the tail)
    }
    LT_REQUIRE(false, "model evaluation: kind %d has no closing step", (int)kind);
}

// the refusals of an evaluation up to its softmax scale - nothing is launched before the last of them - and the shapes they are made on
int forward_dims(lt_engine* e, const lt_step_args* a, int use_cfg, hipStream_t s, const PackedDesc* pk, LtEvalKind kind, Dims& dm) {
    const lt_config& c = e->cfg; const VariantDesc& v = e->v;
    const LtEvalTraits kt = lt_eval_traits(kind);
    const int B = a->batch, p = c.patch_size;
    if (pk) {
        LT_REQUIRE(c.variant == LT_VARIANT_NEXT_T2I, "packed batches: the text-conditional Next-DiT (LT_VARIANT_NEXT_T2I) only; this engine is variant %d", c.variant);
        LT_REQUIRE(pk->tab || !use_cfg, "packed batches: lt_forward_packed is the plain forward (guidance on a size list: lt_forward_cfg_packed)");
        LT_REQUIRE(B >= 1 && B <= c.max_batch && B <= 64, "packed batch of %d exceeds max_batch %d (or 64)", B, c.max_batch);
    }
    LT_REQUIRE(B >= 1 && B <= c.max_batch, "batch %d exceeds max_batch %d", B, c.max_batch);
    LT_REQUIRE(!use_cfg || B % 2 == 0, "forward_with_cfg needs an even batch (cond+uncond)");
    LT_REQUIRE(a->latent_h % p == 0 && a->latent_w % p == 0, "latent %dx%d not divisible by patch", a->latent_h, a->latent_w);
    int Hp = a->latent_h / p, Wp = a->latent_w / p;
    dm.Wrow = v.eol ? Wp + 1 : Wp;  // (Flag-DiT appends one eol token per latent row, model.py:779-786)
    int N = Hp * dm.Wrow;
    if (pk) {  // N = the longest sequence; a->latent_h / latent_w are ignored
        N = 0; Hp = 0; Wp = 0;
        for (int b = 0; b < B; ++b) {
            const int hb = pk->hw[2 * b], wb = pk->hw[2 * b + 1];
            LT_REQUIRE(hb > 0 && wb > 0 && hb % p == 0 && wb % p == 0, "packed sample %d: latent %dx%d not divisible by patch", b, hb, wb);
            dm.ntok[b] = (hb / p) * (wb / p);
            dm.gw[b] = wb / p;
            N = std::max(N, dm.ntok[b]); Hp = std::max(Hp, hb / p); Wp = std::max(Wp, wb / p);
        }
        for (int b = 0; b < B; ++b) dm.pk_full = dm.pk_full && dm.ntok[b] == N;
        dm.ntok_dev = pk->tab ? pk->tab + LT_PK_NTOK * LT_PK_MAX : e->pk_dev;  // (flat form: the entry point stored the table; pointer form: embed_patches copies)
        dm.gw_dev = pk->tab ? pk->tab + LT_PK_GW * LT_PK_MAX : e->pk_dev + 64;
        dm.nk_dev = pk->tab && dm.pk_full ? nullptr : dm.ntok_dev;
    }
    dm.B = B; dm.N = N; dm.Npad = round_up(N, 64); dm.M = B * N; dm.Hp = Hp; dm.Wp = Wp;
    LT_REQUIRE(N <= c.max_tokens, "%d latent tokens exceed max_tokens %d", N, c.max_tokens);
    if (v.rope_1d) LT_REQUIRE(N <= e->rope_len, "sequence of %d tokens exceeds the 1-D RoPE table (%d)", N, e->rope_len);
    else LT_REQUIRE(Hp <= e->rope_len && Wp <= e->rope_len, "latent grid exceeds the RoPE table (%d)", e->rope_len);
    LT_REQUIRE(a->io_dtype == LT_BF16 || a->io_dtype == LT_F32, "io_dtype must be bf16 or f32");
    // (the conditioning buffers are batch-major: the first B rows of one prepared for 2 B are what a preparation of those rows alone leaves)
    LT_REQUIRE(e->prompt_B == B || (kt.half && e->prompt_B == 2 * B), "%s was called for batch %d, step has batch %d",
               v.labels ? "lt_prepare_labels" : "lt_prepare_prompt", e->prompt_B, kt.half ? 2 * B : B);
    LT_REQUIRE(e->reg_Y == 0 || (B == 2 && !pk), "regional captions: one image per call (batch 2 = cond + uncond row), tensor input");
    LT_REQUIRE(e->skip.empty() || (!pk && (int)e->skip.size() < e->L), "layer skip: a tensor input and a set that leaves a layer (SkipScope::set)");
    LT_REQUIRE(e->skip.empty() || kt.skip_ok, "layer skip: a layer-skip set is not served by an evaluation of kind %d", (int)kind);
    LT_REQUIRE(e->perturb.empty() || !pk, "perturbed attention: a packed batch is not served (tensor input only)");
    LT_REQUIRE(e->perturb.empty() || kt.skip_ok, "perturbed attention: a perturb set is not served by an evaluation of kind %d", (int)kind);
    LT_REQUIRE(e->perturb.empty() || e->reg_Y == 0, "perturbed attention: a regional prompt is prepared (lt_prepare_prompt_regional), which is not served");
    LT_REQUIRE(e->blur.empty() || !pk, "blurred queries: a packed batch is not served (tensor input only)");
    LT_REQUIRE(e->blur.empty() || kt.skip_ok, "blurred queries: a blur set is not served by an evaluation of kind %d", (int)kind);
    LT_REQUIRE(e->blur.empty() || e->reg_Y == 0, "blurred queries: a regional prompt is prepared (lt_prepare_prompt_regional), which is not served");
    LT_REQUIRE(e->blur.empty() || e->perturb.empty(), "blurred queries: a blur set together with a perturb set is not served");
    LT_REQUIRE(e->blur.empty() || (e->q_blur && e->blur_taps), "blurred queries: the buffers are not allocated (ensure_blur)");
    LT_REQUIRE(e->blur.empty() || e->blur_mode == 1 || e->blur_radius < std::min(Hp, Wp), "blurred queries: radius %d cannot be reflected on this "
               "call's grid of %d x %d image tokens (radius <= min(rows, columns) - 1)", e->blur_radius, Hp, Wp);
    if (lt_slg_kernel_mode(kind) >= 0) LT_REQUIRE(e->g_skip, "skip-layer guidance: the buffer is not allocated (ensure_skip_buf)");
    if (kind == LT_KIND_REUSE_STORE || kind == LT_KIND_REUSE_AGAIN) LT_REQUIRE(e->g_delta, "guidance reuse: the buffer is not allocated (ensure_delta)");
    LT_REQUIRE(e->rule_form == 0 || (kind == LT_KIND_RULE && e->p_mom && e->p_par && e->p_stats) || kind == LT_KIND_COND_ONLY,
               "projected guidance: form %d on an evaluation of kind %d, or the buffers are not allocated (ensure_project)", e->rule_form, (int)kind);
    e->cache_head[0] = 0;  // (this evaluation rewrites e->x / e->h / e->mod, or uses them up; forward_graphed sets it behind a head)
    if (kt.cached) {
        LT_REQUIRE(!e->moe_rec_on && !e->moe_force_rows, "step caching: MoE routing record / force is not served");
        LT_REQUIRE(e->reg_Y == 0, "step caching: a regional prompt is not served");
        if (!e->tally && refuse_if_capturing(s, "step caching")) return 2;  // (e->tally: the engine's own capture, which is how a part replays)
        LT_REQUIRE(e->c_hprev && e->c_x0 && e->c_r && e->c_ws, "step caching: the buffers are not allocated (ensure_step_cache)");
    }
    if (!e->weights_ok && lt_weights_ready(e)) return 2;
    return 0;
}

// patchify + x_embedder (model.py:777-779) in the three input forms [+ eol token per row] -> e->x
int embed_patches(lt_engine* e, const Dims& dm, const void* x_in, const lt_step_args* a, int use_cfg, const PackedDesc* pk, hipStream_t s) {
    const lt_config& c = e->cfg;
    const int B = dm.B, N = dm.N, p = c.patch_size;
    if (ProfScope ps(e, 2, 0, s); !pk) {
        if (launch_patchify(x_in, a->io_dtype, e->patches, B, c.in_channels, a->latent_h, a->latent_w, p, e->kpad, use_cfg, dm.Wrow, s)) return 1;
    } else if (pk->tab) {  // one launch for all samples
        if (launch_patchify_packed(pk->x_flat, a->io_dtype, e->patches, pk->tab, B, c.in_channels, p, e->kpad, N, use_cfg, s)) return 1;
    } else {
        for (int b = 0; b < B; ++b)
            if (launch_patchify(pk->x_ptrs[b], a->io_dtype, e->patches + (size_t)b * N * e->kpad, 1, c.in_channels, pk->hw[2 * b], pk->hw[2 * b + 1], p, e->kpad, 0, 0, s)) return 1;
        memcpy(e->pk_host, dm.ntok, B * sizeof(int)); memcpy(e->pk_host + 64, dm.gw, B * sizeof(int));
        LT_CHECK_HIP(hipMemcpyAsync(e->pk_dev, e->pk_host, 128 * sizeof(int), hipMemcpyHostToDevice, s));
    }
    if (gemm(e, e->patches, e->kpad, e->xemb_w, e->kpad, e->x, e->d, dm.M, e->d, e->kpad, e->xemb_b, 0, s)) return 1;
    if (pk) {  // padded positions hold the learned pad_token, not an embedded patch (model.py:811-817)
        ProfScope ps(e, 2, 0, s);
        if (pk->tab && !dm.pk_full && launch_fill_pad_packed(e->x, e->pad_token, pk->tab, B, N, e->d, s)) return 1;
        for (int b = 0; !pk->tab && b < B; ++b)
            if (dm.ntok[b] < N && launch_fill_rows_bf16(e->x + ((size_t)b * N + dm.ntok[b]) * e->d, e->pad_token, N - dm.ntok[b], e->d, s)) return 1;
    }
    if (e->v.eol) {
        ProfScope ps(e, 2, 0, s);
        if (launch_eol_fill(e->x, e->eol_token, B * dm.Hp, dm.Wp, e->d, s)) return 1;
    }
    return 0;
}

// conditioning: t_embedder (model.py:84-87) + caption / label embedding (hoisted) -> adaLN vectors of every layer + final (e->mod)
int condition(lt_engine* e, const Dims& dm, const float* t_dev, hipStream_t s) {
    const VariantDesc& v = e->v;
    const int B = dm.B, L = e->L, A = e->A;
    ProfScope ps(e, 2, 0, s);
    const int fused_pro = lt_opt(OPT_PROLOGUE_FUSED);  // round 6, bit mask: 1 timestep features, 2 temb + embedding, 4 prep_mod - each one launch less, bit-identical (LinearSmallMExtra)
    if (fused_pro & 1) { LinearSmallMExtra x; x.t = t_dev; if (launch_linear_small_m_ext(nullptr, e->t0_w, e->t0_b, e->t1, B, A, 256, 0, x, s)) return 1; }
    else if (launch_timestep_features(t_dev, 0, e->tfeat, B, 256, s) || launch_linear_small_m(e->tfeat, e->t0_w, e->t0_b, e->t1, B, A, 256, 0, s)) return 1;
    if (launch_linear_small_m(e->t1, e->t2_w, e->t2_b, e->temb, B, A, A, 1, s)) return 1;
    if (e->gate_t_all && launch_linear_small_m(e->temb, e->gate_t_all, nullptr, e->moe_logits, B, L * e->E, A, 0, s)) return 1;  // every layer's time-router logits
    if (e->moe_tp_live) {  // ... and every layer's time plan: they depend on nothing else (one launch instead of L)
        MoeArgs m;
        m.x = nullptr; m.gate_w = nullptr; m.forced = nullptr; m.sample_logits = e->moe_logits; m.sample_ld = L * e->E;
        m.rows = dm.M; m.rows_per_sample = dm.N; m.d = e->d; m.E = e->E;
        m.sel = e->moe_tp_sel; m.pos = e->moe_tp_pos; m.wts = e->moe_tp_wts; m.src = e->moe_tp_src; m.tile_expert = e->moe_tp_tile_expert;
        m.max_tiles = moe_tiles_for(e, dm.M);
        m.layers = L; m.layer_stride_rows = (long long)e->moe_tp_stride_rows; m.layer_stride_src = (long long)e->moe_tp_stride_src; m.layer_stride_tiles = e->moe_tiles;
        if (launch_moe_plan(m, s)) return 1;
    }
    // once per (sample, channel) instead of once per token inside the row kernels: tanh of the gate chunks (where the
    // family has it) and bf16(1 + scale) of every scale chunk
    unsigned tanh_mask = 0, scale_mask = 0;
    for (int i = 0; i < 2; ++i) {
        if (v.gate_tanh && v.i_gate[i] >= 0) tanh_mask |= 1u << v.i_gate[i];
        if (v.i_scale[i] >= 0) scale_mask |= 1u << v.i_scale[i];
    }
    if (e->cfg.variant == LT_VARIANT_NEXT_MOE) { tanh_mask |= 1u << 5; scale_mask |= 1u << 4; }  // the space branch's chunks
    const int fin2 = v.final_chunks == 2 ? 1 : 0;
    LinearSmallMExtra x;
    const u16* in = e->temb;
    if (fused_pro & 2) x.a2 = e->cap_emb;
    else { if (launch_add_bf16(e->temb, e->cap_emb, e->adaln_in, (long long)B * A, s)) return 1; in = e->adaln_in; }
    if (fused_pro & 4) { x.pm_L = L; x.pm_chunks = e->chunks; x.pm_d = e->d; x.pm_final = fin2; x.pm_tanh = tanh_mask; x.pm_scale = scale_mask; }
    if (fused_pro & 6 ? launch_linear_small_m_ext(in, e->adaln_w, e->adaln_b, e->mod, B, e->ld_mod, A, 1, x, s)
                      : launch_linear_small_m(in, e->adaln_w, e->adaln_b, e->mod, B, e->ld_mod, A, 1, s)) return 1;
    if (!(fused_pro & 4) && launch_prep_mod(e->mod, B, e->ld_mod, L, e->chunks, e->d, tanh_mask, scale_mask, fin2, s)) return 1;
    return 0;
}

// ---- the route of a transformer block ------------------------------------------------------------------
// text keys ride in the self-attention launch (zero-init gated text cross-attention, model.py:420-434); a regional prompt has its own launches
bool fuses_text(const lt_engine* e) { return e->v.text && !(e->reg_Y > 0) && attention_fuses_text(e->hd); }
// the self-attention call of the layer with weights w, as the dispatch predicates and the block see it (raw queries: the block adds q_raw)
AttnArgs self_attn_args(const lt_engine* e, const Dims& dm, const LayerW& w) {
    AttnArgs at;
    at.q = e->q; at.k = e->k; at.vt = e->vt; at.bias = nullptr; at.out = e->attn; at.gate = nullptr; at.accumulate = 0;
    at.B = dm.B; at.H = e->H; at.Hkv = e->Hkv; at.N = dm.N; at.Nk = dm.N; at.Nkpad = dm.Npad; at.hd = e->hd; at.scale = dm.sm_scale; at.k_prescaled = 1;
    at.nk_batch = dm.nk_dev; at.tail_ws = e->attn_tail_ws; at.tail_ws_bytes = e->attn_tail_ws_bytes;
    if (fuses_text(e)) { at.tk = w.ky; at.tvt = w.vty; at.tbias = e->txt_bias; at.tgate = w.gate; at.Tk = e->prompt_T; at.Tkpad = e->prompt_Tpad; }
    return at;
}
// ... and its Q | K | V projection with the V^T image as the second output (the routes that do not take it clear VT)
GemmArgs qkv_gemm_args(const lt_engine* e, const Dims& dm, const LayerW& w) {
    GemmArgs gq;
    gq.A = e->h; gq.W = w.wqkv; gq.C = e->qkv; gq.bias = nullptr; gq.bias_dtype = -1; gq.M = dm.M; gq.N = e->d + 2 * e->dkv; gq.K = e->d;
    gq.lda = e->d; gq.ldw = e->d; gq.ldc = e->qkvn; gq.VT = e->vt; gq.vt_split = e->d + e->dkv; gq.vt_tokens = dm.N; gq.vt_hd = e->hd; gq.vt_npad = dm.Npad;
    return gq;
}

// Kernel-selection options (options.h; lt_set_option = process default, lt_engine_set_option = per-engine override) pick among these:
// QKV_SMALL_FUSED  attn_small_fused, round 5, the class-conditional 600M models at <= 512 tokens: q_norm, k_norm, RoPE, the V transpose and the
//                  attention are ONE launch behind the small-M QKV GEMM, whose epilogue leaves the LayerNorm partials (AttnSmallArgs / GemmArgs::rowstat)
// QKV_FUSED        qkv_fused_gemm: Q | K | V in ONE launch where the shapes are whole tiles of the persistent 256 x 288 kernel: Q | K tiles with the
//                  plain epilogue, V tiles with swapped MFMA operands and the V^T epilogue
// QKV_QK_AND_VT    qkv_vt_epilogue: the V projection is its own GEMM launch whose epilogue writes the attention kernels' V^T image (no v_transpose
//                  pass: 15.6 us per layer at cfg 2, and the 37.7 MB V slice is never written row-major / re-read);  QKV_PLAIN  one GEMM, V transposed behind it
enum QkvRoute { QKV_SMALL_FUSED, QKV_FUSED, QKV_QK_AND_VT, QKV_PLAIN };
// POST_K_ONLY      raw_q: the attention prologue does the queries, the K pass reduces their LayerNorm partials
// POST_ONE_LAUNCH  qkv_post_fused 1, or 2 (default) below 2048 rows: q / k post-processing + V transpose in one launch where the problem is
//                  launch-bound (the three passes are 5 us each at 512 rows - profiles/r02/rocprofv3_kernel_stats_cfg1_r02.csv; bandwidth-bound
//                  problems: three launches are 0.1-0.2 ms / NFE faster, profiles/r01/bench_ab_qkv_post_fused.log)
// POST_QK_PAIR     qk_post_pair, from 2048 rows: q and k share one persistent launch [+ V transpose];  POST_SEPARATE  one launch each
enum PostRoute { POST_K_ONLY, POST_ONE_LAUNCH, POST_QK_PAIR, POST_SEPARATE };
struct BlockPlan {
    bool regional, fuse_text;  // compositional Next-DiT: per-caption text attention + region combine / text keys inside the self-attention launch
    bool pk_one_wave;  // a packed batch whose attention runs on the hd-72 one-wave kernel (the PerSampleKeys instantiation of attention_v4.hip)
    // V^T epilogue: large problems only (a second launch of a latency-bound 512-row GEMM costs more than the transpose), whole 64-key tiles per
    // sample (no key padding to zero); packed batches: when the attention masks their pad rows' keys itself (pk_one_wave), else the transpose kernels
    bool vt_epi;
    QkvRoute qkv;
    // attn_q_fused, round 4: with the fused launch the Q columns' LayerNorm partial sums leave the GEMM epilogue (qstat_slots per row; bn: the tile width) and
    // the attention prologue does q_norm + RoPE itself (AttnArgs::q_raw) - where the hd-72 one-wave kernel takes the call (whole tiles, no packed batch: one
    // rope_grid_w per launch), the RoPE is 2-D, qk_norm is on, the text keys are fused into the launch or absent, and the prompt is not regional
    bool raw_q;
    int bn, qstat_slots;
    PostRoute post;
    // pair_layout, round 6: when every GEMM of the dense block runs on the persistent kernel (>= one tile per CU: the fused QKV launch,
    // O, W1 | W3, W2) and the attention on a one-wave kernel, their A operands and the four weights are kept in the row-pair-interleaved layout
    // (GemmArgs::pair_ab) - bit-identical to the row-major path.  Packed batches take it, and the V^T epilogue, under pk_one_wave: the pad rows'
    // K / V words are pad_token pushed through finite weights and a masked key's weight is an exact zero, so nothing has to zero them.
    bool pair;
    // the MoE families: the experts' grouped GEMMs on the persistent kernel (>= 1.5 tiles per CU) read their weights, and e->moe_us between the
    // two, in the pair layout; the W1 | W3 launch gathers its A rows from e->h, which stays row-major (a gathered row's line mate is no neighbour)
    bool pair_moe;
};

// Decided once, before the first block, on layer 0's weights: the dispatch predicates ask about shapes, which all layers share
int plan_block(const lt_engine* e, const Dims& dm, bool packed, BlockPlan& p) {
    const lt_config& c = e->cfg; const VariantDesc& v = e->v;
    const int M = dm.M, N = dm.N, d = e->d, dkv = e->dkv, hd = e->hd, F = e->F;
    const LayerW& w = e->lw[0];
    p = BlockPlan{}; p.regional = v.text && e->reg_Y > 0; p.fuse_text = fuses_text(e);
    const AttnArgs at = self_attn_args(e, dm, w);
    const GemmArgs gq = qkv_gemm_args(e, dm, w);
    // (head_dim 72 only: a packed batch at another head dim keeps the launches it had, also when every sample has the longest length)
    p.pk_one_wave = packed && hd == 72 && N % 64 == 0 && attention_one_wave_hd72(at);
    p.vt_epi = lt_opt(OPT_QKV_VT_EPILOGUE) && (!packed || p.pk_one_wave) && N % 64 == 0 && (long long)((M + 255) / 256) * ((dkv + 255) / 256) >= 128;
    GemmArgs gs = gq;
    gs.VT = nullptr;  // (the small-M launch has no second output)
    const bool small_fused = lt_opt(OPT_ATTN_SMALL_FUSED) && !v.text && c.qk_norm && !v.rope_1d && !packed && !p.vt_epi &&
                             attention_small_fusable(hd, N, e->H, e->Hkv, d, dkv) && gemm_is_small_m(gs, 0);
    p.qkv = small_fused ? QKV_SMALL_FUSED : p.vt_epi && lt_opt(OPT_QKV_FUSED_GEMM) && gemm_qkv_fusable(gq) ? QKV_FUSED : p.vt_epi ? QKV_QK_AND_VT : QKV_PLAIN;
    if (p.qkv == QKV_FUSED) {
        p.bn = gemm_qkv_tile_width(gq);
        p.raw_q = lt_opt(OPT_ATTN_Q_FUSED) && c.qk_norm && !v.rope_1d && !packed && !p.regional && (p.fuse_text || !v.text) && attention_takes_raw_q(at) &&
                  p.bn > 0 && d % p.bn == 0 && 2 * d / p.bn <= 32;
        if (p.raw_q) p.qstat_slots = 2 * d / p.bn;
    }
    p.post = p.raw_q ? POST_K_ONLY
             : !p.vt_epi && (lt_opt(OPT_QKV_POST_FUSED) == 1 || (lt_opt(OPT_QKV_POST_FUSED) == 2 && M < 2048)) ? POST_ONE_LAUNCH
             : lt_opt(OPT_QK_POST_PAIR) && M >= 2048 ? POST_QK_PAIR : POST_SEPARATE;
    if (lt_opt(OPT_PAIR_LAYOUT) && e->E == 0 && (!packed || p.pk_one_wave) && M % 2 == 0 && d % 32 == 0 && F % 32 == 0 && F <= 16384 && d <= 16384 && !p.regional &&
        (!v.text || attention_fuses_text(hd))) {
        GemmArgs go, g13, g2;
        go.A = e->attn; go.W = w.wo; go.C = e->o; go.bias = nullptr; go.bias_dtype = -1; go.M = M; go.N = d; go.K = d; go.lda = d; go.ldw = d; go.ldc = d;
        g13 = go; g13.A = e->h; g13.W = w.w13; g13.C = e->u; g13.N = 2 * F; g13.ldc = F;
        g2 = go; g2.A = e->u; g2.W = w.w2; g2.K = F; g2.lda = F; g2.ldw = F;
        p.pair = p.qkv == QKV_FUSED && gemm_runs_w4q_dense(go, 0) && gemm_runs_w4q_dense(g13, 1) && gemm_runs_w4q_dense(g2, 0) && attention_is_one_wave(at);
    }
    if (lt_opt(OPT_PAIR_LAYOUT) && e->E > 0 && d % 32 == 0 && F % 32 == 0 && F <= 16384 && d <= 16384) {
        GemmArgs g13, g2;
        moe_gemm_args(e, w.w13_t ? w.w13_t : w.w13_s, w.w2_t ? w.w2_t : w.w2_s, e->moe_tile_expert, e->moe_src, M, g13, g2);
        p.pair_moe = gemm_runs_w4q_grouped(g13, 1) && gemm_runs_w4q_grouped(g2, 0);
    }
    // a graph the caller recorded replays without the engine hearing of it, so it must never meet weights in the other layout: from the first
    // recorded evaluation on (layout_pinned, set by run_forward) every evaluation runs on row-major weights (ensure_weight_layout)
    if (e->layout_pinned) { p.pair = false; p.pair_moe = false; }
    LT_REQUIRE(!p.pair || (p.qkv == QKV_FUSED && !p.regional && (p.fuse_text || !v.text)), "pair layout: the block left the path it was chosen for");
    return 0;
}

// Perturbed attention: the deviations of a layer whose self-attention map is the identity, decided once next to the block's plan.
// Such a layer never takes a V^T-epilogue route (QKV_FUSED / QKV_QK_AND_VT leave V as the transposed image only): it projects plainly -
//   no text:  V alone (the dkv rows of wqkv from row d + dkv on) -> e->qkv as [M][dkv]; the identity launch -> e->attn
//   text:     Q | K | V in one plain launch (K is computed and not read: Q's and V's rows of wqkv are not adjacent, and one launch over the
//             contiguous matrix costs less than two), q_norm + RoPE on Q, the identity launch, then the stand-alone text launch in accumulate mode
// Where the block's plan is QKV_FUSED the projection runs on the persistent kernel (variant 15) in BOTH operand layouts, so the pair plan and
// the row-major plan launch one kernel and their words agree; elsewhere the launcher chooses as always.  Under the pair plan e->h and the
// weights are in the pair layout (pair_ab 3); without text the identity launch writes e->attn in that layout, with text the generic text
// launch accumulates into row-major rows and the O projection reads a row-major A (pair_ab bit 1 alone) - the same products in the same order.
struct PerturbPlan {
    bool text = false;
    int variant = 0, pair_ab = 0;
    bool out_pair = false;     // e->attn leaves the identity launch in the pair layout
    bool attn_rowmajor = false;  // the pair plan's O projection reads e->attn row-major in this layer
};
int plan_perturbed(const lt_engine* e, const BlockPlan& bp, PerturbPlan& pp) {
    pp = PerturbPlan{};
    pp.text = e->v.text;
    LT_REQUIRE(!bp.regional, "perturbed attention: a regional prompt is not served");
    if (bp.qkv == QKV_FUSED) {
        LT_REQUIRE(e->d % 64 == 0 && e->d >= 192, "perturbed attention: d = %d does not fit the persistent kernel the fused plan runs on", e->d);
        pp.variant = 15;
    }
    if (bp.pair) {
        LT_REQUIRE(pp.variant == 15 && (e->d + e->dkv) % 2 == 0, "perturbed attention: the pair plan left the route it was chosen for");
        pp.pair_ab = 3; pp.out_pair = !pp.text; pp.attn_rowmajor = pp.text;
    }
    return 0;
}

int block_attention_perturbed(lt_engine* e, const Dims& dm, const PerturbPlan& pp, LayerW& w, const float* t_dev, const lt_step_args* a, hipStream_t s) {
    const lt_config& c = e->cfg; const VariantDesc& v = e->v;
    const int B = dm.B, N = dm.N, M = dm.M, d = e->d, dkv = e->dkv, H = e->H, Hkv = e->Hkv, hd = e->hd;
    if (!pp.text) {
        if (gemm(e, e->h, d, w.wqkv + (size_t)(d + dkv) * d, d, e->qkv, dkv, M, dkv, d, nullptr, 0, s, nullptr, pp.pair_ab, 0, pp.variant)) return 1;
        ProfScope ps(e, 2, 0, s);
        return launch_attention_identity(e->qkv, dkv, 0, e->attn, B, N, H, Hkv, hd, pp.out_pair, s) ? 1 : 0;
    }
    if (gemm(e, e->h, d, w.wqkv, d, e->qkv, e->qkvn, M, e->qkvn, d, nullptr, 0, s, nullptr, pp.pair_ab, 0, pp.variant)) return 1;
    {
        ProfScope ps(e, 2, 0, s);
        QkPostArgs qa;
        qa.src = e->qkv; qa.ld_src = e->qkvn; qa.B = B; qa.N = N; qa.hd = hd; qa.rope_mode = v.rope_1d ? 2 : 1;
        qa.cs = e->rope; qa.t = t_dev; qa.grid_w = dm.Wp; qa.cs_len = e->rope_len; qa.ln_eps = 1e-5f;
        qa.n_tok_b = dm.ntok_dev; qa.grid_w_b = dm.gw_dev;
        qa.watershed = c.variant == LT_VARIANT_NEXT_T2I ? a->scale_watershed : 0.f;
        qa.col0 = 0; qa.heads = H; qa.dst = e->q; qa.ln_w = c.qk_norm ? w.q_norm_w : nullptr; qa.ln_b = c.qk_norm ? w.q_norm_b : nullptr;
        if (launch_qk_norm_rope(qa, s)) return 1;
        if (launch_attention_identity(e->qkv, e->qkvn, d + dkv, e->attn, B, N, H, Hkv, hd, 0, s)) return 1;
    }
    // the zero-init gated text cross-attention on top, as the stand-alone text launch of block_attention does it
    AttnArgs tx;
    tx.q = e->q; tx.k = w.ky; tx.vt = w.vty; tx.bias = e->txt_bias; tx.out = e->attn; tx.gate = w.gate; tx.accumulate = 1;
    tx.B = B; tx.H = H; tx.Hkv = Hkv; tx.N = N; tx.Nk = e->prompt_T; tx.Nkpad = e->prompt_Tpad; tx.hd = hd; tx.k_prescaled = 1;
    tx.scale = (float)(1.0 / std::sqrt((double)hd)); tx.nk_batch = nullptr;
    return attention(e, tx, s) ? 1 : 0;
}

// Blurred queries (smoothed-energy guidance): the deviations of a layer whose self-attention reads Gaussian-blurred queries, decided
// once next to the block's plan.  Such a layer projects Q | K | V on the plan's GEMM route (QKV_SMALL_FUSED: the plain GEMM and the ordinary
// post-processing - the one-launch attention has its queries in registers only), never hands raw queries to the attention prologue (the K pass
// runs alone, q_norm + RoPE on Q is the stand-alone launch into e->q), blurs e->q into e->q_blur and runs the self-attention on that.  The text
// keys do not ride in that launch: the stand-alone text launch accumulates on top with the UNBLURRED e->q, as a perturbed layer's does - and
// as there it accumulates into row-major rows, so under the pair plan a text layer's self launch writes row-major and the O projection reads
// a row-major A (pair_ab bit 1 alone); without text the attention writes out_pair as the plan does.
struct BlurPlan {
    QkvRoute qkv = QKV_PLAIN;
    PostRoute post = POST_SEPARATE;
    bool text = false;
    bool out_pair = false;       // e->attn leaves the self-attention launch in the pair layout
    bool attn_rowmajor = false;  // the pair plan's O projection reads e->attn row-major in this layer
};
int plan_blurred(const lt_engine* e, const Dims& dm, const BlockPlan& bp, BlurPlan& bl) {
    bl = BlurPlan{};
    bl.text = e->v.text;
    LT_REQUIRE(!bp.regional, "blurred queries: a regional prompt is not served");
    bl.qkv = bp.qkv == QKV_SMALL_FUSED ? QKV_PLAIN : bp.qkv;
    // (what plan_block chooses without raw queries; POST_K_ONLY stays: there it names "the K pass alone", and Q gets its own launch)
    bl.post = bp.post == POST_K_ONLY ? POST_K_ONLY
              : !bp.vt_epi && (lt_opt(OPT_QKV_POST_FUSED) == 1 || (lt_opt(OPT_QKV_POST_FUSED) == 2 && dm.M < 2048)) ? POST_ONE_LAUNCH
              : lt_opt(OPT_QK_POST_PAIR) && dm.M >= 2048 ? POST_QK_PAIR : POST_SEPARATE;
    if (bp.pair) {
        AttnArgs at = self_attn_args(e, dm, e->lw[0]);
        at.q = e->q_blur; at.tk = nullptr; at.tvt = nullptr; at.tbias = nullptr; at.tgate = nullptr; at.Tk = 0; at.Tkpad = 0;
        bl.out_pair = !bl.text && attention_is_one_wave(at);
        bl.attn_rowmajor = !bl.out_pair;
    }
    return 0;
}

// the attention branch of a block up to e->attn: QKV projection, q / k post-processing, self-attention [+ text keys], on the plan's route
// bl: the layer's queries are blurred - the deviations of BlurPlan; null: the block as it is
int block_attention(lt_engine* e, const Dims& dm, const BlockPlan& bp, LayerW& w, const float* t_dev, const lt_step_args* a, hipStream_t s,
                    const BlurPlan* bl = nullptr) {
    const lt_config& c = e->cfg; const VariantDesc& v = e->v;
    const int B = dm.B, N = dm.N, Npad = dm.Npad, M = dm.M, d = e->d, dkv = e->dkv, H = e->H, Hkv = e->Hkv, hd = e->hd;
    GemmArgs gq = qkv_gemm_args(e, dm, w);
    AttnArgs at = self_attn_args(e, dm, w);
    const QkvRoute qkv = bl ? bl->qkv : bp.qkv;
    const PostRoute post = bl ? bl->post : bp.post;
    const bool raw_q = bp.raw_q && !bl;
    if (qkv == QKV_SMALL_FUSED) {
        gq.VT = nullptr; gq.rowstat = e->qstat; gq.rowstat_slots = e->qstat_slots;
        if (profiled_gemm(e, gq, 0, 2.0 * M * (double)(d + 2 * dkv) * d, s)) return 1;
        AttnSmallArgs as;
        as.qkv = e->qkv; as.ld = e->qkvn; as.q_col0 = 0; as.k_col0 = d; as.v_col0 = d + dkv; as.out = e->attn; as.B = B; as.H = H; as.Hkv = Hkv; as.N = N; as.hd = hd;
        as.rowstat = e->qstat; as.slots = e->qstat_slots; as.q_slot0 = 0; as.q_nslot = d / 128; as.k_slot0 = d / 128; as.k_nslot = dkv / 128;
        as.q_ln_w = w.q_norm_w; as.q_ln_b = w.q_norm_b; as.k_ln_w = w.k_norm_w; as.k_ln_b = w.k_norm_b; as.ln_eps = 1e-5f;
        as.cs = e->rope; as.t = t_dev; as.watershed = 0.f; as.cs_len = e->rope_len; as.grid_w = dm.Wp; as.k_scale = dm.sm_scale * LOG2E;
        prefetch_rider(e, &as.pf, e->attn, d, w.wo, d, e->o, d, M, d, d, 0);
        ProfScope ps(e, 1, 4.0 * B * H * (double)N * N * hd, s);
        return launch_attention_small(as, s) ? 1 : 0;  // (class-conditional: no text keys behind it)
    }
    if (qkv == QKV_FUSED) {
        if (raw_q) { gq.qstat = e->qstat; gq.qstat_cols = d; gq.qstat_slots = bp.qstat_slots; }
        gq.pair_ab = bp.pair ? 3 : 0;
        if (profiled_gemm(e, gq, 3, 2.0 * M * (double)(d + 2 * dkv) * d, s)) return 1;
    } else if (qkv == QKV_QK_AND_VT) {
        if (gemm(e, e->h, d, w.wqkv, d, e->qkv, e->qkvn, M, d + dkv, d, nullptr, 0, s)) return 1;
        GemmArgs g;
        g.A = e->h; g.W = w.wqkv + (size_t)(d + dkv) * d; g.C = e->vt; g.bias = nullptr; g.bias_dtype = -1;
        g.M = M; g.N = dkv; g.K = d; g.lda = d; g.ldw = d; g.ldc = 0; g.vt_tokens = N; g.vt_hd = hd; g.vt_npad = Npad;
        if (profiled_gemm(e, g, 2, 2.0 * M * (double)dkv * d, s)) return 1;
    } else if (gemm(e, e->h, d, w.wqkv, d, e->qkv, e->qkvn, M, e->qkvn, d, nullptr, 0, s)) return 1;
    {
        ProfScope ps(e, 2, 0, s);
        QkPostArgs qa;
        qa.src = e->qkv; qa.ld_src = e->qkvn; qa.B = B; qa.N = N; qa.hd = hd; qa.rope_mode = v.rope_1d ? 2 : 1;
        qa.cs = e->rope; qa.t = t_dev; qa.grid_w = dm.Wp; qa.cs_len = e->rope_len; qa.ln_eps = 1e-5f;
        qa.n_tok_b = dm.ntok_dev; qa.grid_w_b = dm.gw_dev;
        qa.watershed = c.variant == LT_VARIANT_NEXT_T2I ? a->scale_watershed : 0.f;  // other families: one table (branch 1)
        QkvPostArgs pa;
        qa.col0 = 0; qa.heads = H; qa.dst = e->q; qa.ln_w = c.qk_norm ? w.q_norm_w : nullptr; qa.ln_b = c.qk_norm ? w.q_norm_b : nullptr;
        pa.q = qa;
        qa.col0 = d; qa.heads = Hkv; qa.dst = e->k; qa.ln_w = c.qk_norm ? w.k_norm_w : nullptr; qa.ln_b = c.qk_norm ? w.k_norm_b : nullptr;
        qa.out_scale = dm.sm_scale * LOG2E;  // softmax scale folded into K's one bf16 rounding (scores in log2 units)
        pa.k = qa;
        pa.v_src = e->qkv; pa.v_dst = e->vt; pa.v_ld_src = e->qkvn; pa.v_col0 = d + dkv; pa.v_B = B; pa.v_N = N; pa.v_Npad = Npad; pa.v_kv_heads = Hkv; pa.v_hd = hd;
        if (post == POST_K_ONLY && !raw_q) {  // a blurred layer of the raw-query plan: the K pass alone, the queries in a launch of their own
            if (launch_qk_norm_rope(pa.k, s) || launch_qk_norm_rope(pa.q, s)) return 1;
        } else if (post == POST_K_ONLY) {
            pa.k.qstat_in = e->qstat; pa.k.qstat_out = e->qmr; pa.k.qstat_slots = bp.qstat_slots; pa.k.qstat_width = d;
            if (launch_qk_norm_rope(pa.k, s)) return 1;
            at.q = nullptr; at.q_raw = e->qkv; at.q_ld = e->qkvn; at.q_col0 = 0; at.q_stat = e->qmr; at.q_ln_w = w.q_norm_w; at.q_ln_b = w.q_norm_b;
            at.rope_cs = e->rope; at.rope_cs_t = e->rope_tr; at.rope_t = t_dev; at.rope_watershed = pa.q.watershed; at.rope_cs_len = e->rope_len; at.rope_grid_w = dm.Wp;
        } else if (post == POST_ONE_LAUNCH) {
            if (!bl && !bp.regional && (bp.fuse_text || !v.text)) prefetch_rider(e, &pa.pf, e->attn, d, w.wo, d, e->o, d, M, d, d, 0);
            if (launch_qkv_post(pa, s)) return 1;
        } else {
            if (post == POST_QK_PAIR) { if (launch_qk_norm_rope_pair(pa.q, pa.k, s)) return 1; }
            else if (launch_qk_norm_rope(pa.q, s) || launch_qk_norm_rope(pa.k, s)) return 1;
            if (!bp.vt_epi && launch_v_transpose(e->qkv, e->qkvn, d + dkv, e->vt, B, N, Npad, Hkv, hd, s)) return 1;
        }
    }
    at.out_pair = bl ? bl->out_pair : bp.pair;
    if (bl) {  // e->q -> e->q_blur, the self-attention on the blurred queries without the text keys
        ProfScope ps(e, 2, 0, s);
        if (launch_query_blur(e->q, e->q_blur, e->blur_taps, B, H, N, hd, dm.Wrow, dm.Wp, e->blur_radius, e->blur_mode, s)) return 1;
        at.q = e->q_blur; at.tk = nullptr; at.tvt = nullptr; at.tbias = nullptr; at.tgate = nullptr; at.Tk = 0; at.Tkpad = 0;
    }
    if (attention(e, at, s)) return 1;
    if (bp.regional || (v.text && (bl || !bp.fuse_text))) {  // the text keys in launches of their own
        AttnArgs tx = at;
        tx.q = e->q; tx.out_pair = 0;  // (a blurred layer: the text keys see the queries as they are)
        tx.k = w.ky; tx.vt = w.vty; tx.bias = e->txt_bias; tx.nk_batch = nullptr;
        tx.Nk = e->prompt_T; tx.Nkpad = e->prompt_Tpad; tx.scale = (float)(1.0 / std::sqrt((double)hd));
        if (!bp.regional) { tx.gate = w.gate; tx.accumulate = 1; return attention(e, tx, s) ? 1 : 0; }
        // compositional Next-DiT (lumina_next_compositional_generation/models/model.py:422-446): every caption attends the queries of its row (regional
        // captions -> cond row 0, last -> uncond row 1) into its own buffer, then one pass applies region masks, tanh(gate), the caption sum and the residual add
        tx.B = e->reg_Y; tx.q_batch_map = e->reg_qmap; tx.gate = nullptr; tx.accumulate = 0; tx.out = e->reg_txt;
        if (attention(e, tx, s)) return 1;
        ProfScope ps(e, 2, 0, s);
        if (launch_region_text_combine(e->attn, e->reg_txt, w.gate, e->reg_Y, N, H, hd, dm.Hp, dm.Wp, e->reg_h, e->reg_w, s)) return 1;
    }
    return 0;
}

// block l on the plan's route; h leaves prepared for layer nl, the next one that runs (L: none does - the final layer's form)
// pp: the layer is perturbed - its attention branch up to e->attn is block_attention_perturbed's; everything behind is the block as it is
int run_block(lt_engine* e, const Dims& dm, const BlockPlan& bp, int l, int nl, const float* t_dev, const lt_step_args* a, hipStream_t s,
              const PerturbPlan* pp = nullptr, const BlurPlan* bl = nullptr) {
    const VariantDesc& v = e->v;
    const int B = dm.B, N = dm.N, M = dm.M, d = e->d, F = e->F, pair = bp.pair;
    const int post_mode = v.post ? 1 : 0, gate_mode = 0;  // gates arrive ready (tanh applied by the conditioning where the family has it)
    LayerW& w = e->lw[l];
    if (pp ? block_attention_perturbed(e, dm, *pp, w, t_dev, a, s) : block_attention(e, dm, bp, w, t_dev, a, s, bl)) return 1;
    int ys_o = 0, ys_f = 0;
    if (gemm(e, e->attn, d, w.wo, d, e->o, d, M, d, d, nullptr, 0, s, &ys_o, pair ? ((pp && pp->attn_rowmajor) || (bl && bl->attn_rowmajor) ? 2 : 3) : 0)) return 1;
    {   // x += gate' * post(attn) ; h = pre_ffn(x) * (1 + scale) [+ shift]
        ProfScope ps(e, 2, 0, s);
        GatedResArgs g = gated_res_args(e, dm);
        if (ys_o) { g.ystat = e->ystat; g.ystat_slots = ys_o; }
        g.y = e->o; g.post_w = v.post ? w.attn_norm2 : nullptr; g.gate = mod_chunk(e, l, v.i_gate[0]);
        g.post_mode = post_mode; g.gate_mode = gate_mode; g.next_mode = 1; g.h_pair = pair;
        g.next_w = v.pre_w ? w.ffn_norm1 : nullptr; g.next_scale = mod_chunk(e, l, v.i_scale[1]); g.next_shift = mod_chunk(e, l, v.i_shift[1]);
        if (e->E == 0) prefetch_rider(e, &g.pf, e->h, d, w.w13, d, e->u, F, M, 2 * F, d, 1);
        if (launch_gated_residual_norm(g, s)) return 1;
    }
    if (e->E == 0) {
        if (gemm(e, e->h, d, w.w13, d, e->u, F, M, 2 * F, d, nullptr, 1, s, nullptr, pair ? 3 : 0, pair)) return 1;
        if (gemm(e, e->u, F, w.w2, F, e->o, d, M, d, F, nullptr, 0, s, &ys_f, pair ? 3 : 0)) return 1;
    } else if (e->moe_mode != 0) {  // one MoE FFN in the ImageNet block (models.py:755-758: time-routed; models1.py: per token)
        if (moe_ffn(e, w, l, e->moe_mode == 1 ? 0 : 1, M, N, B, s, false, bp.pair_moe)) return 1;
    } else {  // time MoE -> residual -> space MoE (models2.py:793-800)
        if (moe_ffn(e, w, l, 0, M, N, B, s, false, bp.pair_moe)) return 1;
        {
            ProfScope ps(e, 2, 0, s);
            GatedResArgs g = gated_res_args(e, dm);
            moe_y(e, g, l); g.post_w = w.norm_time; g.gate = mod_chunk(e, l, 3); g.post_mode = 1; g.gate_mode = 0; g.next_scale = mod_chunk(e, l, 4); g.next_mode = 1;
            // round 5 (option moe_route_fused): h is the space router's input and this kernel holds the row - it routes on its way out
            // (one launch less per layer; moe_route_kernel's arithmetic, statement for statement)
            if (lt_opt(OPT_MOE_ROUTE_FUSED)) {
                g.route_w = w.gate_s; g.route_E = e->E; g.route_sel = e->moe_sel; g.route_wts = e->moe_wts;
                if (e->moe_force_rows) {
                    LT_REQUIRE(e->moe_force_rows == M, "forced MoE routing was given for %d rows, this call has %d", e->moe_force_rows, M);
                    g.route_forced = e->moe_force + ((size_t)l * 2 + 1) * (size_t)e->cfg.max_batch * e->cfg.max_tokens * 2;
                }
            }
            if (launch_gated_residual_norm(g, s)) return 1;
        }
        if (moe_ffn(e, w, l, 1, M, N, B, s, lt_opt(OPT_MOE_ROUTE_FUSED) != 0, bp.pair_moe)) return 1;
    }
    // x += gate' * post(ffn) ; h = next layer's pre-norm + modulate, or the final layer's LayerNorm(no affine, 1e-6) * (1 + scale) [+ shift]
    ProfScope ps(e, 2, 0, s);
    GatedResArgs g = gated_res_args(e, dm);
    g.y = e->o; g.post_w = e->E == 0 ? (v.post ? w.ffn_norm2 : nullptr) : e->moe_mode != 0 ? w.ffn_norm2 : w.norm_space;
    g.gate = mod_chunk(e, l, e->E != 0 && e->moe_mode == 0 ? 5 : v.i_gate[1]);
    if (ys_f) { g.ystat = e->ystat; g.ystat_slots = ys_f; }
    if (e->E != 0) moe_y(e, g, e->moe_mode == 1 ? l : -1);
    g.post_mode = post_mode; g.gate_mode = gate_mode;
    if (nl < e->L) {
        g.next_w = v.pre_w ? e->lw[nl].attn_norm1 : nullptr; g.next_scale = mod_chunk(e, nl, v.i_scale[0]);
        g.next_shift = mod_chunk(e, nl, v.i_shift[0]); g.next_mode = 1; g.h_pair = pair;
        prefetch_rider(e, &g.pf, e->h, d, e->lw[nl].wqkv, d, e->qkv, e->qkvn, M, e->qkvn, d, 0);
    } else { g.next_w = nullptr; g.next_mode = 2; g.next_shift = final_shift(e); g.next_scale = final_scale(e); }
    return launch_gated_residual_norm(g, s) ? 1 : 0;
}

// One evaluation as plain launches: the refusals (forward_dims), [a head: embed_patches, condition,] plan_block + weight layout, [a head: the first
// pre-norm,] run_block for every layer that is not skipped, [a step-caching cut,] the final linear and the closing step.  kind (eval_kind.h): other than
// LT_KIND_WHOLE for a tensor state only.  The three parts of an evaluation under step caching are cut behind the first pre-norm and the last block
int run_forward(lt_engine* e, const void* x_in, const float* t_dev, void* out, const lt_step_args* a, int use_cfg,
                hipStream_t s, const PackedDesc* pk = nullptr, LtEvalKind kind = LT_KIND_WHOLE) {
    const lt_config& c = e->cfg; const VariantDesc& v = e->v;
    const int L = e->L, d = e->d;
    Dims dm;
    if (int rc = forward_dims(e, a, use_cfg, s, pk, kind, dm)) return rc;
    const int B = dm.B, N = dm.N, M = dm.M;
    const bool do_head = lt_eval_traits(kind).reads_x, do_blocks = kind != LT_KIND_CACHE_HEAD && kind != LT_KIND_CACHE_APPLY;
    // the CALLER is recording this evaluation into a graph of its own (e->tally: the capture is the engine's, forward_graphed).  Nothing was
    // launched yet: what cannot be recorded is refused here, and the capture stays valid
    const bool caller_cap = !e->tally && stream_capturing(s);
    if (caller_cap && refuse_profile_if_capturing(e, s, "model evaluation")) return 2;
    if (softmax_scale_for(e, a, N, &dm.sm_scale)) return 1;
    // the last refusal is behind us and the first launch ahead: only an evaluation that IS recorded pins the engine (and before ensure_rope:
    // the table's rebuild is recorded whatever the host believes the table holds)
    if (caller_cap) e->layout_pinned = true;
    if (ensure_rope(e, a, s)) return 1;
    if (do_head && embed_patches(e, dm, x_in, a, use_cfg, pk, s)) return 1;  // (a part behind the head: x_0, h and the modulation are in place)
    // (host state the blocks read: the same for every part of an evaluation, whichever of them ran as plain launches)
    e->moe_tp_live = e->gate_t_all && e->moe_tp_sel && lt_opt(OPT_MOE_TIME_PLAN_HOIST) && !e->moe_force_rows && B <= LT_MOE_PLAN_TIME_MAX_SAMPLES;
    if (do_head && condition(e, dm, t_dev, s)) return 1;
    BlockPlan bp;
    if (int rc = plan_block(e, dm, pk != nullptr, bp)) return rc;
    if (ensure_weight_layout(e, bp.pair || bp.pair_moe, s, caller_cap)) return 1;
    e->last_pair = bp.pair || bp.pair_moe;
    // layer skip: the blocks in e->skip (ascending; a SkipScope of the entry point stored it, checked) are the identity on e->x - they launch
    // nothing, and whoever prepares h prepares it for nx(l), the next layer that runs (L: none does).  Empty set: nx(l) = l + 1, first = 0
    auto skipped = [&](int l) { return std::binary_search(e->skip.begin(), e->skip.end(), l); };
    auto nx = [&](int l) { int n = l + 1; while (n < L && skipped(n)) ++n; return n; };
    const int first = nx(-1);  // (< L: the set is distinct and shorter than L, checked before the first launch)
    // perturbed attention: the blocks in e->perturb (ascending, disjoint from e->skip) run with the identity as their attention map
    PerturbPlan pp;
    if (!e->perturb.empty())
        if (int rc = plan_perturbed(e, bp, pp)) return rc;
    auto perturbed = [&](int l) { return std::binary_search(e->perturb.begin(), e->perturb.end(), l); };
    // blurred queries: the blocks in e->blur (ascending, disjoint from e->skip; e->perturb is empty then) blur their queries
    BlurPlan bl;
    if (!e->blur.empty())
        if (int rc = plan_blurred(e, dm, bp, bl)) return rc;
    auto blurred = [&](int l) { return std::binary_search(e->blur.begin(), e->blur.end(), l); };
    if (do_head) {  // first pre-norm: modulate(attention_norm(x), [shift,] scale) (model.py:599 / models.py:785 / lumina_t2i model.py:600)
        ProfScope ps(e, 2, 0, s);
        NormModArgs n;
        n.x = e->x; n.w = v.pre_w ? e->lw[first].attn_norm1 : nullptr; n.scale = mod_chunk(e, first, v.i_scale[0]); n.shift = mod_chunk(e, first, v.i_shift[0]);
        n.out = e->h; n.rows = M; n.rows_per_batch = N; n.d = d; n.ld_mod = e->ld_mod; n.eps = c.norm_eps; n.scale_pre = 1; n.out_pair = bp.pair;
        if (launch_rmsnorm_mod(n, s)) return 1;
    }
    if (kind == LT_KIND_CACHE_HEAD) {  // step caching, first cut: the indicator on h (in the layout this key's evaluations leave it in), x_0 kept
        ProfScope ps(e, 2, 0, s);
        if (launch_cache_indicator(e->h, e->c_hprev, (long long)M * d, e->c_ws, e->c_ws + 2 * LT_CACHE_BLOCKS, s)) return 1;
        LT_CHECK_HIP(hipMemcpyAsync(e->c_x0, e->x, (size_t)M * d * sizeof(u16), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    for (int l = do_blocks ? first : L; l < L; l = nx(l))
        if (int rc = run_block(e, dm, bp, l, nx(l), t_dev, a, s, perturbed(l) ? &pp : nullptr, blurred(l) ? &bl : nullptr)) return rc;
    if (kind == LT_KIND_CACHE_BLOCKS) {  // step caching, second cut: r = bfr(x_L - x_0) for the evaluations that leave the stack out
        ProfScope ps(e, 2, 0, s);
        if (launch_cache_residual_store(e->x, e->c_x0, e->c_r, (long long)M * d, s)) return 1;
    } else if (kind == LT_KIND_CACHE_APPLY) {  // ... and such an evaluation: x = bfr(x_0 + r), then what the last block's closing kernel does to x_L
        ProfScope ps(e, 2, 0, s);
        if (launch_cache_residual_apply(e->x, e->c_r, final_scale(e), final_shift(e), e->ld_mod, e->h, M, N, d, s)) return 1;
    }
    if (gemm(e, e->h, d, e->final_w, d, e->frows, e->nfinal, M, e->nfinal, d, e->final_b, 0, s)) return 1;
    ProfScope ps(e, 2, 0, s);  // the closing step, in the input's form
    if (!pk) return close_forward(e, out, a, use_cfg, B, dm.Wrow, kind, s) ? 1 : 0;
    if (pk->tab)
        return launch_unpatchify_packed(e->frows, e->nfinal, pk->out_flat, a->io_dtype, pk->tab, B, c.in_channels, c.out_channels, c.patch_size, N, use_cfg,
                                        a->cfg_scale, cfg_channels(a), s) ? 1 : 0;
    for (int b = 0; b < B; ++b)  // x[i][:L] -> [C, H_b, W_b], sigma half dropped (model.py:757-768, :859-864)
        if (launch_unpatchify_cfg(e->frows + (size_t)b * N * e->nfinal, e->nfinal, pk->out_ptrs[b], a->io_dtype, 1, c.in_channels,
                                  c.out_channels, pk->hw[2 * b], pk->hw[2 * b + 1], c.patch_size, 0, 1.0f, cfg_channels(a), 0, s)) return 1;
    return 0;
}

// One model evaluation through a cached HIP graph.  The first call for a key runs eagerly (it also performs the one-time
// hipFuncSetAttribute calls of the launchers), the second captures the same launch sequence on the engine's private stream
// with the staging buffers as input / output and instantiates it, later calls replay: copy in, one graph launch, copy out.
// Kernel arguments are baked into a graph, so the key holds everything they depend on: the step arguments (shapes, cfg scale,
// RoPE scaling, softmax scale inputs), the prompt dimensions, cfg on / off and the option generation.  Weights and prompt
// CONTENTS live behind fixed pointers and may change freely.
// profiling brackets launches with HIP events, which a graph cannot carry: while an enabled class still has event budget left the
// evaluation runs eagerly; once the budgets are used up replays resume and only add their launch / flop counts (lt_profile_read
// scales the measured time by launches / bracketed launches - every evaluation has the same launch mix)
bool profiling_wants_events(const lt_engine* e) {
    if (!e->prof_on) return false;
    for (int k = 0; k < 3; ++k) {
        const ProfClass& pc = e->prof[k];
        if (((e->prof_mask >> k) & 1) && pc.used < std::min(pc.ev.size(), pc.budget)) return true;  // (also before the window opens)
    }
    return false;
}

}  // namespace

bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

int refuse_if_capturing(hipStream_t s, const char* who) {
    LT_REQUIRE(!stream_capturing(s), "%s: refused on a stream under capture: the call allocates, synchronises or copies from host memory, which a "
               "graph cannot replay (and which would end the capture with an error) - make it before the capture begins", who);
    return 0;
}

// a bf16 buffer [max_batch / 2, in_channels, max_tokens patch^2] the closing kernels of guidance reuse / skip-layer guidance keep between two
// evaluations: allocated by the first call that needs it and kept for the engine's life (captured graphs hold the pointer)
static int ensure_half_state(lt_engine* e, u16** buf, const char* what) {
    if (*buf) return 0;
    const lt_config& c = e->cfg;
    const size_t words = (size_t)(c.max_batch / 2) * c.in_channels * c.max_tokens * c.patch_size * c.patch_size;
    LT_REQUIRE(words > 0, "%s: an engine of max_batch %d holds no cond + uncond pair", what, c.max_batch);
    void* q = nullptr;
    if (dev_alloc(e, &q, words * sizeof(u16), false)) return 1;  // (never read before an evaluation of the same call wrote it)
    *buf = (u16*)q;
    return 0;
}

// the buffers of projected guidance: the momentum (zeroed by every call that starts one), the partial sums and the parameter words
int ensure_project(lt_engine* e) {
    if (e->p_mom && e->p_stats && e->p_par) return 0;
    const lt_config& c = e->cfg;
    const size_t words = (size_t)(c.max_batch / 2) * c.in_channels * c.max_tokens * c.patch_size * c.patch_size;
    LT_REQUIRE(words > 0, "projected guidance: an engine of max_batch %d holds no cond + uncond pair", c.max_batch);
    void* q = nullptr;
    if (!e->p_mom) { if (dev_alloc(e, &q, words * sizeof(float))) return 1; e->p_mom = (float*)q; }
    if (!e->p_stats) { if (dev_alloc(e, &q, (size_t)(c.max_batch / 2) * LT_GUIDANCE_SLICES * LT_PROJECT_SUMS * sizeof(double))) return 1; e->p_stats = (double*)q; }
    if (!e->p_par) { if (dev_alloc(e, &q, 4 * sizeof(float))) return 1; e->p_par = (float*)q; }
    return 0;
}

int ensure_delta(lt_engine* e) { return ensure_half_state(e, &e->g_delta, "guidance reuse"); }
int ensure_skip_buf(lt_engine* e) { return ensure_half_state(e, &e->g_skip, "skip-layer guidance"); }

// one layer set (what: "skip" / "perturb"): count, range, repeats
static int check_layer_set(const lt_engine* e, const char* who, const char* what, const int32_t* host, int n) {
    LT_REQUIRE(n >= 0, "%s: n_%s %d is negative", who, what, n);
    LT_REQUIRE(n == 0 || host, "%s: null argument (%s_host: %d layer indices)", who, what, n);
    LT_REQUIRE(n <= e->L, "%s: %d %s indices, the model has %d layers", who, n, what, e->L);
    for (int i = 0; i < n; ++i) {
        LT_REQUIRE(host[i] >= 0 && host[i] < e->L, "%s: %s index %d (entry %d) is outside 0..%d", who, what, host[i], i, e->L - 1);
        for (int j = 0; j < i; ++j) LT_REQUIRE(host[j] != host[i], "%s: %s index %d is repeated (entries %d and %d)", who, what, host[i], j, i);
    }
    return 0;
}

int check_layer_sets(const lt_engine* e, const char* who, const int32_t* skip_host, int n_skip, const int32_t* perturb_host, int n_perturb) {
    if (check_layer_set(e, who, "skip", skip_host, n_skip)) return 2;
    LT_REQUIRE(n_skip < e->L, "%s: the skip set leaves no layer (all %d are in it)", who, e->L);
    if (check_layer_set(e, who, "perturb", perturb_host, n_perturb)) return 2;  // (may hold every layer)
    for (int i = 0; i < n_perturb; ++i)
        for (int j = 0; j < n_skip; ++j)
            LT_REQUIRE(perturb_host[i] != skip_host[j], "%s: layer %d is in the skip set and in the perturb set (the sets are disjoint)", who, perturb_host[i]);
    return 0;
}

int check_skip_set(const lt_engine* e, const char* who, const int32_t* skip_host, int n_skip) {
    return check_layer_sets(e, who, skip_host, n_skip, nullptr, 0);
}

int SkipScope::set(const char* who, const int32_t* skip_host, int n_skip, const int32_t* perturb_host, int n_perturb) {
    if (check_layer_sets(e, who, skip_host, n_skip, perturb_host, n_perturb)) return 2;
    e->skip.assign(skip_host, skip_host + n_skip);
    std::sort(e->skip.begin(), e->skip.end());
    e->perturb.assign(perturb_host, perturb_host + n_perturb);
    std::sort(e->perturb.begin(), e->perturb.end());
    return 0;
}

int check_blur_sets(const lt_engine* e, const char* who, const int32_t* skip_host, int n_skip, const int32_t* blur_host, int n_blur, float sigma) {
    if (check_layer_set(e, who, "skip", skip_host, n_skip)) return 2;
    LT_REQUIRE(n_skip < e->L, "%s: the skip set leaves no layer (all %d are in it)", who, e->L);
    if (check_layer_set(e, who, "blur", blur_host, n_blur)) return 2;  // (may hold every layer)
    for (int i = 0; i < n_blur; ++i)
        for (int j = 0; j < n_skip; ++j)
            LT_REQUIRE(blur_host[i] != skip_host[j], "%s: layer %d is in the skip set and in the blur set (the sets are disjoint)", who, blur_host[i]);
    LT_REQUIRE(n_blur == 0 || sigma > 0.f, "%s: blur sigma %g is not positive (+inf is the mean query)", who, (double)sigma);
    return 0;
}

int check_blur_radius(const lt_engine* e, const char* who, const lt_step_args* a, int n_blur, float sigma) {
    if (n_blur <= 0) return 0;
    float taps[2 * LT_SEG_MAX_RADIUS + 1];
    int r = 0, mode = 0;
    LT_REQUIRE(seg_taps_host(sigma, taps, &r, &mode) == 0, "%s: blur sigma %g is not positive (+inf is the mean query)", who, (double)sigma);
    const int p = e->cfg.patch_size, Hp = p > 0 ? a->latent_h / p : 0, Wp = p > 0 ? a->latent_w / p : 0;
    LT_REQUIRE(mode == 1 || r < std::min(Hp, Wp), "%s: blur radius %d (sigma %g) cannot be reflected on this call's grid of %d x %d image tokens "
               "(radius <= min(rows, columns) - 1)", who, r, (double)sigma, Hp, Wp);
    return 0;
}

int SkipScope::set_blur(const char* who, const int32_t* skip_host, int n_skip, const int32_t* blur_host, int n_blur) {
    if (check_blur_sets(e, who, skip_host, n_skip, blur_host, n_blur, 1.f)) return 2;
    e->skip.assign(skip_host, skip_host + n_skip);
    std::sort(e->skip.begin(), e->skip.end());
    e->blur.assign(blur_host, blur_host + n_blur);
    std::sort(e->blur.begin(), e->blur.end());
    return 0;
}

int ensure_blur(lt_engine* e, float sigma, hipStream_t s) {
    float taps[2 * LT_SEG_MAX_RADIUS + 1] = {0.f};
    int r = 0, mode = 0;
    LT_REQUIRE(seg_taps_host(sigma, taps, &r, &mode) == 0, "blurred queries: sigma %g is not positive", (double)sigma);
    void* q = nullptr;
    if (!e->q_blur) {  // (never read before the blur of the same layer wrote it)
        if (dev_alloc(e, &q, (size_t)e->cfg.max_batch * e->cfg.max_tokens * e->d * sizeof(u16), false)) return 1;
        e->q_blur = (u16*)q;
    }
    if (!e->blur_taps) { if (dev_alloc(e, &q, sizeof taps)) return 1; e->blur_taps = (float*)q; }
    LT_CHECK_HIP(hipMemcpyAsync(e->blur_taps, taps, sizeof taps, hipMemcpyHostToDevice, s));
    LT_CHECK_HIP(hipStreamSynchronize(s));  // taps is a stack temporary
    e->blur_mode = mode; e->blur_radius = r;
    return 0;
}

int refuse_profile_if_capturing(const lt_engine* e, hipStream_t s, const char* who) {
    if (!(e->prof_on && e->prof_mask)) return 0;
    LT_REQUIRE(!stream_capturing(s), "%s: refused on a stream under capture while lt_profile_enable is on (the profile brackets launches with "
               "events, which a graph cannot carry): switch the profile off before the capture", who);
    return 0;
}

int softmax_scale_for(const lt_engine* e, const lt_step_args* a, int N, float* scale) {
    const int hd = e->hd;
    if (a->proportional_attn && !e->v.labels) {
        LT_REQUIRE(a->base_seqlen > 1, "proportional_attn needs base_seqlen");
        const double lg = std::log((double)N) / std::log((double)a->base_seqlen);
        if (e->softmax_rule == LT_SOFTMAX_ANAGRAM) {
            // the fork walks the queries in int(seqlen / base_seqlen + 0.99) chunks of base_seqlen rows (nextdit.py:336-352, :390); every chunk
            // sees all keys, so a row's result does not depend on the chunking - unless the chunks end before the rows do
            const long long chunks = (long long)((double)N / (double)a->base_seqlen + 0.99);
            LT_REQUIRE(chunks * a->base_seqlen >= N, "LT_SOFTMAX_ANAGRAM: %lld query chunks of base_seqlen %d do not cover %d tokens (the reference's "
                       "chunk loop drops the last %lld query rows at this shape)", chunks, a->base_seqlen, N, (long long)N - chunks * a->base_seqlen);
            // math.log(seqlen, base_seqlen) / math.sqrt(head_dim)  (nextdit.py:333)
            *scale = (float)(lg / std::sqrt((double)hd));
        } else {
            // math.sqrt(math.log(seqlen, base_seqlen) / head_dim)  (model.py:374; seqlen counts the eol tokens for Flag-DiT)
            *scale = (float)std::sqrt(lg / (double)hd);
        }
    } else {
        *scale = (float)std::sqrt(1.0 / (double)hd);  // model.py:376; flash_attn_func default (models.py:389)
    }
    return 0;
}

static int forward_graphed_body(lt_engine* e, const void* x_in, const float* t_dev, void* out, const lt_step_args* a, int use_cfg, hipStream_t s,
                               const EvalSpec& spec) {
    const PackedCall* pc = spec.pc;
    const LtEvalKind kind = spec.kind;
    const LtEvalTraits kt = lt_eval_traits(kind);
    // a stage of the guidance schedule: the scale travels through e->g_cfg - on the eager path too, so both run one kernel - and the key
    // holds a zeroed cfg_scale; a half-row kind has a->batch / 2 rows (B' rows evaluated, 2 B' written)
    lt_step_args own;
    if (kt.dev_scale) {
        LT_REQUIRE(!pc && a->batch % 2 == 0, "a guidance schedule needs a tensor state with an even batch");
        own = *a;
        own.cfg_scale = 0.f;
        if (kt.half) own.batch = a->batch / 2;
        if (kind != LT_KIND_COND_ONLY && spec.cfg_dev != e->g_cfg)
            LT_CHECK_HIP(hipMemcpyAsync(e->g_cfg, spec.cfg_dev, sizeof(float), hipMemcpyDeviceToDevice, s));
        a = &own;
        use_cfg = kt.half ? 0 : 1;
    }
    // one evaluation as plain launches; a packed batch's flat state goes through the ragged kernels
    auto run = [&](const void* x, const float* t, void* o, hipStream_t st) {
        if (!pc) return run_forward(e, x, t, o, a, use_cfg, st, nullptr, kind);
        PackedDesc pk{nullptr, nullptr, pc->hw};
        pk.x_flat = x; pk.out_flat = o; pk.tab = e->pk_tab;
        return run_forward(e, nullptr, t, nullptr, a, use_cfg, st, &pk);
    };
    if (!lt_opt(OPT_GRAPH) || profiling_wants_events(e) || e->moe_rec_on || e->moe_force_rows) return run(x_in, t_dev, out, s);
    const int B = a->batch;
    // "graph" 2 (default): replay above 1024 rows only.  At 512 rows a replay (three staging copies + the graph launch) costs more than it
    // saves - plain launches are 1.5-4.6 % faster for the 600M ImageNet model, same box (profiles/r05/bench_ab_hip_graph_on_off_cfg1_cfg5.log:
    // 1.652 against 1.68-1.73 ms per NFE; the MoE model is neutral) - and the host issues its ~125 launches per evaluation in a quarter of
    // the time the GPU needs for them.  Above that the two are equal and the graph keeps a busy host out of the picture.
    if (lt_opt(OPT_GRAPH) == 2 && pc && (long long)B * pc->n_max <= 1024) return run(x_in, t_dev, out, s);
    if (lt_opt(OPT_GRAPH) == 2 && !pc && a->latent_h > 0 && a->latent_w > 0 && e->cfg.patch_size > 0 &&
        (long long)B * (a->latent_h / e->cfg.patch_size) * (a->latent_w / e->cfg.patch_size) <= 1024)
        return run(x_in, t_dev, out, s);
    if (B < 1 || B > e->cfg.max_batch || (!pc && (a->latent_h <= 0 || a->latent_w <= 0)) || (a->io_dtype != LT_BF16 && a->io_dtype != LT_F32))
        return run(x_in, t_dev, out, s);  // let the eager path produce the error message
    const size_t sbytes = (pc ? (size_t)pc->elems : (size_t)B * e->cfg.in_channels * a->latent_h * a->latent_w) * (a->io_dtype == LT_BF16 ? 2 : 4);
    const size_t cap_bytes = (size_t)e->cfg.max_batch * e->cfg.in_channels * e->cfg.max_tokens * e->cfg.patch_size * e->cfg.patch_size * 4;
    if ((kt.half ? 2 * sbytes : sbytes) > cap_bytes) return run(x_in, t_dev, out, s);
    // a caller that is capturing ITS stream (torch.cuda.graph around the sampler) cannot launch a graph or start a second capture
    // from inside: hand it plain launches, which its own capture records.  The cache is not touched: a key first seen here would be pinned to
    // the row-major regime of a recorded evaluation (ge->pair) for callers that never capture
    if (stream_capturing(s)) return run(x_in, t_dev, out, s);
    // (both option generations: the process defaults' and this engine's overrides' - kernel selection is baked into a captured graph)
    // ... and the softmax rule: the scale it selects is a kernel argument (qa.out_scale / at.scale)
    // ... and the kind: every kind is another launch sequence or another closing kernel (what a kind reads from device memory - the scale,
    // the rule's parameters - is no part of the key)
    const int extra[11] = {use_cfg, e->prompt_B, e->prompt_T, e->prompt_Tpad, e->reg_Y, e->reg_h, e->reg_w, lt_opt_generation(), lt_opt_engine_generation(),
                           e->softmax_rule, (int)kind};
    std::vector<char> key(sizeof(lt_step_args) + sizeof(extra));
    memcpy(key.data(), a, sizeof(lt_step_args));
    memcpy(key.data() + sizeof(lt_step_args), extra, sizeof(extra));
    if (pc) key.insert(key.end(), (const char*)pc->hw, (const char*)(pc->hw + 2 * B));  // the size list: grids and the table's contents depend on it
    if (!e->skip.empty()) {  // the layers left out: another launch sequence.  Behind a -1 no size list holds; empty: the key of always
        const int32_t mark[2] = {-1, (int32_t)e->skip.size()};
        key.insert(key.end(), (const char*)mark, (const char*)(mark + 2));
        key.insert(key.end(), (const char*)e->skip.data(), (const char*)(e->skip.data() + e->skip.size()));
    }
    if (!e->perturb.empty()) {  // the layers perturbed, behind a mark of their own: skip {1} and perturb {1} are two keys
        const int32_t mark[2] = {-2, (int32_t)e->perturb.size()};
        key.insert(key.end(), (const char*)mark, (const char*)(mark + 2));
        key.insert(key.end(), (const char*)e->perturb.data(), (const char*)(e->perturb.data() + e->perturb.size()));
    }
    if (!e->blur.empty()) {  // the layers with blurred queries, behind a mark of their own, with what sigma stands for but the taps
        const int32_t mark[4] = {-4, (int32_t)e->blur.size(), (int32_t)e->blur_mode, (int32_t)e->blur_radius};
        key.insert(key.end(), (const char*)mark, (const char*)(mark + 4));
        key.insert(key.end(), (const char*)e->blur.data(), (const char*)(e->blur.data() + e->blur.size()));
    }
    if (e->rule_form != 0 && kind == LT_KIND_RULE) {  // a projected form: other closing kernels.  Form 0: the key of always
        const int32_t mark[2] = {-3, (int32_t)e->rule_form};
        key.insert(key.end(), (const char*)mark, (const char*)(mark + 2));
    }
    lt_engine::GraphEntry* ge = nullptr;
    for (auto& g : e->graphs) if (g.key == key) { ge = &g; break; }
    if (!ge) {
        if (e->graphs.size() >= 16) {  // bound the cache: drop the oldest entry
            if (e->graphs.front().exec) (void)hipGraphExecDestroy(e->graphs.front().exec);
            e->graphs.erase(e->graphs.begin());
        }
        e->graphs.emplace_back();
        ge = &e->graphs.back();
        ge->key = key;
    }
    if (e->layout_pinned && ge->pair) {  // recorded on pair-layout weights, which the engine no longer holds: start the key over
        if (ge->exec) (void)hipGraphExecDestroy(ge->exec);
        ge->exec = nullptr; ge->uses = 0; ge->failed = false; ge->pair = false;
    }
    if (ge->failed || ge->uses++ == 0) {
        const int rc = run(x_in, t_dev, out, s);
        ge->pair = e->last_pair;  // (the weight layout this key's evaluations run on; a function of the key)
        return rc;
    }
    // the RoPE table is ONE shared buffer outside every graph (it is rebuilt only when scale / ntk change): a replay of key A after
    // key B changed the table must rebuild it first - before every replay, not only before the capture
    if (ensure_rope(e, a, s)) return 1;
    // ... and so are the GEMM weights' layouts (row-major / pair): evaluations of another regime may have converted them since
    if (ensure_weight_layout(e, ge->pair, s)) return 1;
    if (!ge->exec) {
        if (!e->cap_stream) LT_CHECK_HIP(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        bool ok = hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        int rc = 0;
        if (ok) {
            ge->tally = lt_engine::GraphTally();
            e->tally = &ge->tally;
            rc = run(e->g_x, e->g_t, e->g_out, e->cap_stream);
            e->tally = nullptr;
            if (rc == 0 && e->last_pair != ge->pair) { lt_set_error("graph capture: the evaluation's operand layout changed between the eager run and the capture"); rc = 1; }
            ok = hipStreamEndCapture(e->cap_stream, &graph) == hipSuccess && rc == 0 && graph != nullptr;
        }
        if (ok) ok = hipGraphInstantiate(&ge->exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
        if (!ok) {  // capture is an optimisation: fall back to eager launches for this key
            (void)hipGetLastError();
            ge->exec = nullptr;
            ge->failed = true;
            if (rc) return rc;
            return run(x_in, t_dev, out, s);
        }
    }
    // (step caching: the head reads the state, the other two parts do not; the blocks read the times again - staged for every part, so
    //  that no replay depends on which of the evaluation's parts ran as plain launches)
    if (kt.reads_x) LT_CHECK_HIP(hipMemcpyAsync(e->g_x, x_in, sbytes, hipMemcpyDeviceToDevice, s));
    LT_CHECK_HIP(hipMemcpyAsync(e->g_t, t_dev, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, s));
    LT_CHECK_HIP(hipGraphLaunch(ge->exec, s));
    e->last_pair = ge->pair;  // (a replay is an evaluation too: "last_pair" of lt_engine_get_option names the regime of the last one)
    if (kt.writes_out)  // (the skip evaluation's closing kernel writes e->g_skip and nothing else; a step-caching head no output)
        LT_CHECK_HIP(hipMemcpyAsync(out, e->g_out, kt.half ? 2 * sbytes : sbytes, hipMemcpyDeviceToDevice, s));
    ++e->graph_replays;
    if (e->prof_on)
        for (int k = 0; k < 3; ++k)
            if ((e->prof_mask >> k) & 1) { e->prof[k].flops += ge->tally.flops[k]; e->prof[k].launches += ge->tally.launches[k]; }
    return 0;
}

int forward_graphed(lt_engine* e, const void* x_in, const float* t_dev, void* out, const lt_step_args* a, int use_cfg, hipStream_t s,
                    const EvalSpec& spec) {
    // e->cache_head (step caching): which head's e->x / e->h / e->mod are in place.  Kept here, not in run_forward: a replay runs none of
    // run_forward's host code
    const int sig[5] = {a->batch, a->latent_h, a->latent_w, a->io_dtype, use_cfg};
    if (lt_eval_traits(spec.kind).cached) {
        LT_REQUIRE(!spec.pc, "step caching: a packed batch is not served (tensor input only)");
        LT_REQUIRE(spec.kind == LT_KIND_CACHE_HEAD || memcmp(e->cache_head, sig, sizeof sig) == 0, "step caching: this evaluation does not follow "
                   "its probe - the head of an evaluation of the same step arguments, with no other evaluation between");
    }
    e->cache_head[0] = 0;
    const int rc = forward_graphed_body(e, x_in, t_dev, out, a, use_cfg, s, spec);
    if (rc == 0 && spec.kind == LT_KIND_CACHE_HEAD) memcpy(e->cache_head, sig, sizeof sig);
    return rc;
}

// the buffers of step caching: three token streams of the engine's largest evaluation, the indicator's partials with its two
// result words behind them, and the page-locked pair the controller reads
int ensure_step_cache(lt_engine* e) {
    if (e->c_sums_host) return 0;
    const size_t words = (size_t)e->cfg.max_batch * e->cfg.max_tokens * e->d;
    void* q = nullptr;
    if (!e->c_hprev) { if (dev_alloc(e, &q, words * sizeof(u16))) return 1; e->c_hprev = (u16*)q; }  // (zeroed: the first probe reads it)
    if (!e->c_x0) { if (dev_alloc(e, &q, words * sizeof(u16), false)) return 1; e->c_x0 = (u16*)q; }
    if (!e->c_r) { if (dev_alloc(e, &q, words * sizeof(u16), false)) return 1; e->c_r = (u16*)q; }
    if (!e->c_ws) { if (dev_alloc(e, &q, (2 * LT_CACHE_BLOCKS + 2) * sizeof(double))) return 1; e->c_ws = (double*)q; }
    LT_CHECK_HIP(hipHostMalloc((void**)&e->c_sums_host, 2 * sizeof(double), hipHostMallocDefault));
    return 0;
}

// =====================================================================================================
extern "C" int lt_create(const lt_config* cfg, lt_engine** out) {
    LT_REQUIRE(cfg && out, "lt_create: null argument");
    LT_REQUIRE(cfg->variant >= LT_VARIANT_NEXT_T2I && cfg->variant <= LT_VARIANT_NEXT_MOE_SPACE, "lt_create: unknown variant %d", cfg->variant);
    const bool is_moe = cfg->variant == LT_VARIANT_NEXT_MOE || cfg->variant == LT_VARIANT_NEXT_MOE_TIME || cfg->variant == LT_VARIANT_NEXT_MOE_SPACE;
    LT_REQUIRE(!is_moe || (cfg->num_experts >= 2 && cfg->num_experts <= 8),
               "lt_create: the MoE variant needs 2..8 experts (top-2 routing), got %d", cfg->num_experts);
    const VariantDesc vd = variant_desc(cfg->variant);
    LT_REQUIRE(cfg->dim > 0 && cfg->n_layers >= 1 && cfg->n_heads >= 1 && cfg->n_kv_heads >= 1 && cfg->ffn_hidden > 0 && cfg->adaln_dim > 0,
               "lt_create: dim, n_layers, n_heads, n_kv_heads, ffn_hidden and adaln_dim must be positive");
    LT_REQUIRE(cfg->patch_size >= 1 && cfg->in_channels >= 1 && cfg->out_channels >= 1 && cfg->max_tokens >= 1 && cfg->max_text >= 0,
               "lt_create: patch_size, in_channels, out_channels, max_tokens must be positive (max_text >= 0)");
    LT_REQUIRE(cfg->dim % cfg->n_heads == 0, "dim %% n_heads != 0");
    LT_REQUIRE(cfg->n_heads % cfg->n_kv_heads == 0, "n_heads %% n_kv_heads != 0");
    const int hd = cfg->dim / cfg->n_heads;
    LT_REQUIRE(hd == 48 || hd == 72 || hd == 96 || hd == 128, "head_dim %d not built (48, 72, 96, 128)", hd);
    // hd 128 = the 7B factories of the class-conditional and MoE families; no reference model pairs it with a text branch, the attention
    // kernels have no text phase at this head dim and there is no fixture to hold one to
    LT_REQUIRE(hd != 128 || !vd.text, "head_dim 128 with text cross-attention not built (the class-conditional and MoE variants run at head_dim 128)");
    LT_REQUIRE(cfg->dim % 64 == 0 && cfg->ffn_hidden % 64 == 0, "dim and ffn_hidden must be multiples of 64");
    LT_REQUIRE(!vd.text || (cfg->cap_feat_dim % 64 == 0 && cfg->cap_feat_dim > 0), "cap_feat_dim must be a positive multiple of 64");
    LT_REQUIRE(!vd.labels || cfg->num_classes > 0, "class-conditional variant needs num_classes > 0");
    LT_REQUIRE(cfg->dim <= 4096 && cfg->cap_feat_dim <= 4096, "dim / cap_feat_dim above 4096 not supported by the row kernels");
    LT_REQUIRE(cfg->adaln_dim % 8 == 0 && cfg->max_batch >= 1 && cfg->max_batch <= 8, "adaln_dim %% 8 and 1 <= max_batch <= 8 required");
    LT_REQUIRE(cfg->in_channels * cfg->patch_size * cfg->patch_size <= 64, "patch vector longer than 64");
    lt_engine* e = new lt_engine();
    e->cfg = *cfg;
    e->v = vd;
    e->d = cfg->dim; e->L = cfg->n_layers; e->H = cfg->n_heads; e->Hkv = cfg->n_kv_heads; e->hd = hd;
    e->F = cfg->ffn_hidden; e->dkv = e->Hkv * hd; e->qkvn = e->d + 2 * e->dkv; e->A = cfg->adaln_dim;
    e->cap = vd.text ? cfg->cap_feat_dim : 0; e->nfinal = cfg->patch_size * cfg->patch_size * cfg->out_channels;
    e->kpad = 64; e->chunks = vd.chunks; e->ld_mod = e->L * e->chunks * e->d + vd.final_chunks * e->d;
    e->label_rows = vd.labels ? cfg->num_classes + 1 : 0;
    e->E = is_moe ? cfg->num_experts : 0;
    e->moe_mode = cfg->variant == LT_VARIANT_NEXT_MOE_TIME ? 1 : (cfg->variant == LT_VARIANT_NEXT_MOE_SPACE ? 2 : 0);
    // 2-D RoPE: positions per axis (384, model.py:734); 1-D: one position per token of the longest sequence
    e->rope_len = vd.rope_1d ? round_up(cfg->max_tokens, 64) : (cfg->rope_table_len > 0 ? cfg->rope_table_len : 384);
    const int d = e->d, L = e->L, F = e->F, dkv = e->dkv, A = e->A, cap = e->cap, H = e->H, Hkv = e->Hkv;
    e->lw.resize(L);
    auto fail = [&]() { lt_destroy(e); return 1; };
#define A16(ptr, n) do { void* _p; if (dev_alloc(e, &_p, (size_t)(n) * 2)) return fail(); (ptr) = (u16*)_p; } while (0)
    const int Tmax = round_up(cfg->max_text > 0 ? cfg->max_text : 64, 64);
    for (int l = 0; l < L; ++l) {
        LayerW& w = e->lw[l];
        A16(w.wqkv, (size_t)e->qkvn * d); A16(w.wo, (size_t)d * d);
        if (e->E == 0) { A16(w.w13, (size_t)2 * F * d); A16(w.w2, (size_t)d * F); }
        else {
            const size_t E_ = e->E;
            if (e->moe_mode != 2) {
                A16(w.w13_t, E_ * 2 * F * d); A16(w.w2_t, E_ * d * F);
                // the time routers of ALL layers are one [L * E, A] matrix: their logits depend on the timestep embedding only, so one GEMV
                // per evaluation computes every layer's (run_forward; 16 launches of 12 us each at the 600M model before round 5)
                if (l == 0) A16(e->gate_t_all, (size_t)L * E_ * A);
                w.gate_t = e->gate_t_all + (size_t)l * E_ * A;
            }
            if (e->moe_mode != 1) { A16(w.w13_s, E_ * 2 * F * d); A16(w.w2_s, E_ * d * F); A16(w.gate_s, E_ * d); }
            A16(w.norm_time, d); A16(w.norm_space, d);
        }
        A16(w.q_norm_w, d); A16(w.q_norm_b, d); A16(w.k_norm_w, dkv); A16(w.k_norm_b, dkv);
        A16(w.attn_norm1, d); A16(w.attn_norm2, d); A16(w.ffn_norm1, d); A16(w.ffn_norm2, d);
        if (vd.text) {
            A16(w.wkvy, (size_t)2 * dkv * cap); A16(w.ky_norm_w, dkv); A16(w.ky_norm_b, dkv); A16(w.gate, H); A16(w.y_norm, cap);
            A16(w.ky, (size_t)cfg->max_batch * Hkv * Tmax * hd); A16(w.vty, (size_t)cfg->max_batch * Hkv * hd * Tmax);
        }
        char key[128];
        std::vector<const char*> names = {"attention.wq.weight", "attention.wk.weight", "attention.wv.weight", "attention.wo.weight",
                                          "adaLN_modulation.1.weight", "adaLN_modulation.1.bias"};
        if (e->E == 0) for (const char* nm : {"feed_forward.w1.weight", "feed_forward.w2.weight", "feed_forward.w3.weight"}) names.push_back(nm);
        if (vd.text) for (const char* nm : {"attention.wk_y.weight", "attention.wv_y.weight", "attention.gate", "attention_y_norm.weight"}) names.push_back(nm);
        if (cfg->variant == LT_VARIANT_NEXT_T2I)
            for (const char* nm : {"attention_norm1.weight", "attention_norm2.weight", "ffn_norm1.weight", "ffn_norm2.weight"}) names.push_back(nm);
        else if (cfg->variant == LT_VARIANT_NEXT_MOE)
            for (const char* nm : {"attention_norm.weight", "ffn_norm_time.weight", "ffn_norm_space.weight",
                                   "feed_forward_time.gate.weight", "feed_forward_space.gate.weight"}) names.push_back(nm);
        else if (e->moe_mode != 0)
            for (const char* nm : {"attention_norm.weight", "ffn_norm.weight", "feed_forward.gate.weight"}) names.push_back(nm);
        else
            for (const char* nm : {"attention_norm.weight", "ffn_norm.weight"}) names.push_back(nm);
        if (cfg->qk_norm) {
            for (const char* nm : {"attention.q_norm.weight", "attention.q_norm.bias", "attention.k_norm.weight", "attention.k_norm.bias"}) names.push_back(nm);
            if (vd.text) for (const char* nm : {"attention.ky_norm.weight", "attention.ky_norm.bias"}) names.push_back(nm);
        }
        for (const char* nm : names) { snprintf(key, sizeof(key), "layers.%d.%s", l, nm); e->need[key] = false; }
        for (int ex = 0; ex < e->E; ++ex)
            for (const char* br : {"feed_forward_time", "feed_forward_space"})
                for (const char* wn : {"w1", "w2", "w3"}) {
                    if (e->moe_mode != 0 && br[13] == 's') continue;  // one MoeLayer: keys "feed_forward.experts..."
                    snprintf(key, sizeof(key), "layers.%d.%s.experts.%d.%s.weight", l, e->moe_mode != 0 ? "feed_forward" : br, ex, wn);
                    e->need[key] = false;
                }
    }
    A16(e->xemb_w, (size_t)d * e->kpad); A16(e->xemb_b, d); A16(e->t0_w, (size_t)A * 256); A16(e->t0_b, A);
    A16(e->t2_w, (size_t)A * A); A16(e->t2_b, A); A16(e->pad_token, d);
    if (vd.text) { A16(e->capln_w, cap); A16(e->capln_b, cap); A16(e->cape_w, (size_t)A * cap); A16(e->cape_b, A); }
    if (vd.labels) A16(e->label_table, (size_t)e->label_rows * A);
    if (vd.eol) A16(e->eol_token, d);
    A16(e->adaln_w, (size_t)e->ld_mod * A); A16(e->adaln_b, e->ld_mod);
    A16(e->final_w, (size_t)e->nfinal * d); A16(e->final_b, e->nfinal);
    for (const char* nm : {"x_embedder.weight", "x_embedder.bias", "t_embedder.mlp.0.weight", "t_embedder.mlp.0.bias",
                           "t_embedder.mlp.2.weight", "t_embedder.mlp.2.bias", "final_layer.linear.weight", "final_layer.linear.bias",
                           "final_layer.adaLN_modulation.1.weight", "final_layer.adaLN_modulation.1.bias"})
        e->need[nm] = false;
    if (vd.text) for (const char* nm : {"cap_embedder.0.weight", "cap_embedder.0.bias", "cap_embedder.1.weight", "cap_embedder.1.bias"}) e->need[nm] = false;
    if (vd.labels) e->need["y_embedder.embedding_table.weight"] = false;
    if (vd.eol) e->need["eol_token"] = false;
    // workspace
    const size_t Bm = cfg->max_batch, Nm = cfg->max_tokens, M = Bm * Nm;
    const size_t Npad = round_up((int)Nm, 64);
    A16(e->x, M * d); A16(e->h, M * d); A16(e->qkv, M * e->qkvn); A16(e->q, M * d); A16(e->k, M * dkv);
    A16(e->vt, Bm * Hkv * hd * Npad); A16(e->attn, M * d); A16(e->o, M * d);
    if (e->E == 0) A16(e->u, M * F);
    else {  // expert-sorted buffers: every row appears twice, each expert segment starts on a 256-row tile
        // the experts' W1 | W3 GEMM gathers its rows through ONE buffer descriptor over the FFN input (launch_gemm_bf16: a_row_map):
        // fail here, with the sizes, not at the first forward
        if ((long long)M * d * 2 >= 0x40000000LL) {
            lt_set_error("lt_create: mixture-of-experts engine with max_batch * max_tokens = %zu rows of d = %d: the FFN input (%.2f GB) exceeds "
                         "the 1 GB the gather-on-load GEMM addresses; lower max_batch / max_tokens", M, d, (double)M * d * 2 / 1e9);
            return fail();
        }
        e->moe_tiles = (int)((2 * M + (size_t)e->E * 255 + 255) / 256);
        const size_t P = (size_t)e->moe_tiles * 256;
        A16(e->moe_us, P * F); A16(e->moe_ys, P * d); A16(e->moe_logits, Bm * e->E * (size_t)L); A16(e->moe_wts, 2 * M);
        void* q;
        if (dev_alloc(e, &q, (2 * M + 4) * sizeof(int))) return fail();  // (+4: moe_plan reads / writes whole 16-byte quads)
        e->moe_sel = (int*)q;
        if (dev_alloc(e, &q, (2 * M + 4) * sizeof(int))) return fail();
        e->moe_pos = (int*)q;
        if (dev_alloc(e, &q, (size_t)e->moe_tiles * sizeof(int))) return fail();
        e->moe_tile_expert = (int*)q;
        if (dev_alloc(e, &q, P * sizeof(int))) return fail();
        e->moe_src = (int*)q;
        if (e->moe_mode != 2) {  // per-layer plans of the time router (a few hundred KB per layer at 8192 rows)
            e->moe_tp_stride_rows = 2 * M + 4;
            e->moe_tp_stride_src = P;
            if (dev_alloc(e, &q, (size_t)L * e->moe_tp_stride_rows * sizeof(int))) return fail();
            e->moe_tp_sel = (int*)q;
            if (dev_alloc(e, &q, (size_t)L * e->moe_tp_stride_rows * sizeof(int))) return fail();
            e->moe_tp_pos = (int*)q;
            if (dev_alloc(e, &q, (size_t)L * e->moe_tp_stride_rows * sizeof(u16))) return fail();
            e->moe_tp_wts = (u16*)q;
            if (dev_alloc(e, &q, (size_t)L * e->moe_tiles * sizeof(int))) return fail();
            e->moe_tp_tile_expert = (int*)q;
            if (dev_alloc(e, &q, (size_t)L * P * sizeof(int))) return fail();
            e->moe_tp_src = (int*)q;
        }
    }
    {
        void* q;
        // [rows][slots] float2: 32 slots for the fused QKV launch's Q partials (GemmArgs::qstat), one per 128-column tile of the whole
        // projection for the small-M form (GemmArgs::rowstat)
        e->qstat_slots = std::max(32, (e->qkvn + 127) / 128);
        if (dev_alloc(e, &q, M * (size_t)e->qstat_slots * 2 * sizeof(float))) return fail();
        e->qstat = (float*)q;
        if (dev_alloc(e, &q, M * 2 * sizeof(float))) return fail();
        e->qmr = (float*)q;
        e->ystat_cap = 2 * ((d + 255) / 256);  // two wave halves per 256- or 288-column tile of a d-wide projection
        if (dev_alloc(e, &q, M * (size_t)e->ystat_cap * sizeof(float))) return fail();
        e->ystat = (float*)q;
    }
    if (hd == 96) {  // tail split of the one-wave attention kernel (launch_attention_v4_hd96): up to 4 parts of <= 128 rows per head
        void* q;
        e->attn_tail_ws_bytes = attention_tail_ws_floats((int)Bm * H, 4, 128) * sizeof(float);
        if (dev_alloc(e, &q, e->attn_tail_ws_bytes)) return fail();
        e->attn_tail_ws = (float*)q;
    }
    {   // split-K workspace (zeroed by dev_alloc: the counters must start at 0; every launch leaves them at 0)
        void* q;
        e->splitk_tiles = 256;  // slots of [2][64 x 128] floats (a 64 x 128 tile split two ways; a 128 x 128 tile split four ways takes four)
        if (dev_alloc(e, &q, (size_t)e->splitk_tiles * 2 * 64 * 128 * sizeof(float))) return fail();
        e->splitk_part = (float*)q;
        if (dev_alloc(e, &q, (size_t)e->splitk_tiles * sizeof(unsigned))) return fail();
        e->splitk_cnt = (unsigned*)q;
    }
    if (e->E > 0 && M >= 8192) {  // tail split of the experts' W2 GEMM (GemmArgs::tail_*): only where the grouped persistent kernel can run (>= 1.5 tiles per CU)
        void* q;
        e->tail_cap_parts = 4LL * num_cus();  // up to 4 parts for each of the < #CUs tiles of a partial round: 256 KB each
        if (dev_alloc(e, &q, (size_t)e->tail_cap_parts * 256 * 256 * sizeof(float))) return fail();
        e->tail_part = (float*)q;
        if (dev_alloc(e, &q, (size_t)num_cus() * sizeof(unsigned))) return fail();
        e->tail_cnt = (unsigned*)q;
    }
    A16(e->patches, M * e->kpad); A16(e->frows, M * e->nfinal); A16(e->mod, Bm * e->ld_mod);
    A16(e->tfeat, Bm * 256); A16(e->t1, Bm * A); A16(e->temb, Bm * A);
    A16(e->cap_emb, Bm * A); A16(e->adaln_in, Bm * A);
    if (vd.text) { A16(e->cap_ln, Bm * cap); A16(e->capb, Bm * Tmax * cap); A16(e->capn, Bm * Tmax * cap); A16(e->kvy, Bm * Tmax * 2 * dkv); }
    {
        void* p;
        if (dev_alloc(e, &p, Bm * Tmax * sizeof(float))) return fail();
        e->txt_bias = (float*)p;
        if (dev_alloc(e, &p, (size_t)2 * e->rope_len * (hd / 2) * 2 * sizeof(float))) return fail();
        e->rope = (float*)p;
        if (dev_alloc(e, &p, (size_t)2 * e->rope_len * (hd / 2) * 2 * sizeof(float))) return fail();
        e->rope_tr = (float*)p;
        const size_t state = Bm * cfg->in_channels * Nm * cfg->patch_size * cfg->patch_size * sizeof(float);
        for (int i = 0; i < 2; ++i) { if (dev_alloc(e, &e->ys[i], state)) return fail(); }
        if (dev_alloc(e, &e->ymid, state)) return fail();
        // stage times of the samplers: room for a 256-point grid of 4-stage steps without a (synchronising) reallocation
        if (e->times.create((int)(1024 * Bm))) return fail();
        if (dev_alloc(e, &e->g_x, state)) return fail();
        if (dev_alloc(e, &e->g_out, state)) return fail();
        {
            void* q;
            if (dev_alloc(e, &q, Bm * sizeof(float))) return fail();
            e->g_t = (float*)q;
            if (dev_alloc(e, &q, 4 * sizeof(float))) return fail();  // (the scale; the rescale blend and the norm limit of a rule; the skip-layer scale)
            e->g_cfg = (float*)q;
            if (dev_alloc(e, &q, (size_t)((cfg->max_batch + 1) / 2) * LT_GUIDANCE_SLICES * 4 * sizeof(double))) return fail();
            e->g_stats = (double*)q;
            if (dev_alloc(e, &q, sizeof(int))) return fail();  // (zeroed: the weights start row-major)
            e->w_pair_dev = (int*)q;
        }
        for (int i = 0; i < 4; ++i) { if (dev_alloc(e, &e->kbuf[i], state)) return fail(); }
    }
#undef A16
    *out = e;
    return 0;
}

extern "C" void lt_destroy(lt_engine* e) {
    if (!e) return;
    for (auto& ge : e->graphs) if (ge.exec) (void)hipGraphExecDestroy(ge.exec);
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
    for (auto& b : e->allocs) (void)hipFree(b.p);
    e->times.release();
    e->rk.release();
    if (e->c_sums_host) (void)hipHostFree(e->c_sums_host);
    if (e->pk_dev) (void)hipFree(e->pk_dev);
    if (e->pk_tab) (void)hipFree(e->pk_tab);
    if (e->reg_txt) (void)hipFree(e->reg_txt);
    if (e->reg_qmap) (void)hipFree(e->reg_qmap);
    drop_views(e);
    drop_windows(e);
    if (e->moe_rec) (void)hipFree(e->moe_rec);
    if (e->moe_force) (void)hipFree(e->moe_force);
    for (int k = 0; k < 3; ++k)
        for (auto& pr : e->prof[k].ev) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    delete e;
}

extern "C" int lt_set_weight(lt_engine* e, const char* key, const void* src_dev, int32_t dtype, const int64_t* shape,
                             int32_t ndim, void* stream) {
    LT_REQUIRE(e && key && src_dev && shape, "lt_set_weight: null argument");
    LT_REQUIRE(ndim >= 1 && ndim <= 8, "lt_set_weight: ndim %d outside 1..8", ndim);
    for (int i = 0; i < ndim; ++i) LT_REQUIRE(shape[i] > 0, "weight '%s': shape[%d] = %lld", key, i, (long long)shape[i]);
    if (refuse_if_capturing((hipStream_t)stream, "lt_set_weight")) return 2;  // (a recorded upload would replay from a source long gone)
    Slot s;
    if (find_slot(e, key, &s)) return 2;
    long long n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    LT_REQUIRE(n == (long long)s.rows * s.cols, "weight '%s': %lld elements given, %lld expected (%d x %d)", key, n,
               (long long)s.rows * s.cols, s.rows, s.cols);
    // uploads write row-major rows - after the refusals: a refused upload converts nothing
    if (ensure_weight_layout(e, false, (hipStream_t)stream)) return 1;
    if (launch_upload_rows(src_dev, dtype, s.dst, s.rows, s.cols, s.dst_ld, s.r0, s.row_map, (hipStream_t)stream)) return 1;
    auto it = e->need.find(key);
    if (it != e->need.end()) it->second = true;
    e->weights_ok = false;
    // the hoisted conditioning (text K / V of every layer, caption / label embedding) was computed from the previous weights:
    // the next step must be preceded by a new lt_prepare_prompt / lt_prepare_labels (run_forward refuses otherwise)
    e->prompt_B = 0;
    return 0;
}

extern "C" int lt_weights_ready(lt_engine* e) {
    LT_REQUIRE(e, "null engine");
    for (auto& kv : e->need) LT_REQUIRE(kv.second, "weight '%s' was never uploaded", kv.first.c_str());
    e->weights_ok = true;
    return 0;
}

// per-layer text K / V of `Bc` captions (model.py:421-422, :602): RMSNorm_y -> wk_y | wv_y -> ky_norm, V^T
static int prepare_caption_kv(lt_engine* e, int Bc, int T, int Tpad, hipStream_t s) {
    const lt_config& c = e->cfg;
    const int cap = e->cap, dkv = e->dkv;
    for (int l = 0; l < e->L; ++l) {
        LayerW& w = e->lw[l];
        NormModArgs n;  // attention_y_norm (model.py:602)
        n.x = e->capb; n.w = w.y_norm; n.scale = nullptr; n.shift = nullptr; n.out = e->capn;
        n.rows = Bc * T; n.rows_per_batch = T; n.d = cap; n.ld_mod = 0; n.eps = c.norm_eps;
        if (launch_rmsnorm_mod(n, s)) return 1;
        GemmArgs g;  // wk_y | wv_y (model.py:421-422)
        g.A = e->capn; g.W = w.wkvy; g.C = e->kvy; g.bias = nullptr; g.M = Bc * T; g.N = 2 * dkv; g.K = cap;
        g.lda = cap; g.ldw = cap; g.ldc = 2 * dkv; g.bias_dtype = -1;
        if (launch_gemm_bf16(g, 0, 0, s)) return 1;
        QkPostArgs qa;  // ky_norm, no rotary (model.py:421)
        qa.src = e->kvy; qa.ld_src = 2 * dkv; qa.col0 = 0; qa.B = Bc; qa.N = T; qa.heads = e->Hkv; qa.hd = e->hd;
        qa.rope_mode = 0; qa.cs = nullptr; qa.t = nullptr; qa.grid_w = 1; qa.cs_len = 0; qa.ln_eps = 1e-5f; qa.watershed = 0.f;
        qa.ln_w = c.qk_norm ? w.ky_norm_w : nullptr; qa.ln_b = c.qk_norm ? w.ky_norm_b : nullptr; qa.dst = w.ky;
        qa.out_scale = (float)(1.0 / std::sqrt((double)e->hd)) * LOG2E;  // SDPA default scale (model.py:427-432), folded like the self-attention K
        if (launch_qk_norm_rope(qa, s)) return 1;
        if (launch_v_transpose(e->kvy, 2 * dkv, dkv, w.vty, Bc, T, Tpad, e->Hkv, e->hd, s)) return 1;
    }
    return 0;
}

extern "C" int lt_prepare_prompt(lt_engine* e, const void* cap_feats_dev, int32_t cap_dtype, const int32_t* cap_mask_dev,
                                 int32_t B, int32_t T, void* stream) {
    LT_REQUIRE(e && cap_feats_dev && cap_mask_dev, "lt_prepare_prompt: null argument");
    e->delta_sig[0] = 0;  // (guidance reuse: a stored difference belongs to the conditioning it was taken on)
    e->proj_sig[0] = 0;   // (projected guidance: so does a stored momentum)
    e->cache_res[0] = 0; e->cache_head[0] = 0;  // (step caching: so does a stored residual, and a probe)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(e->v.text, "lt_prepare_prompt: this variant is class-conditional (use lt_prepare_labels)");
    hipStream_t s = (hipStream_t)stream;
    const lt_config& c = e->cfg;
    const int Tmax = round_up(c.max_text > 0 ? c.max_text : 64, 64);
    LT_REQUIRE(B >= 1 && B <= c.max_batch, "prompt batch %d exceeds max_batch %d", B, c.max_batch);
    LT_REQUIRE(T >= 1 && T <= Tmax, "text length %d exceeds max_text %d", T, Tmax);
    LT_REQUIRE(cap_dtype == LT_BF16 || cap_dtype == LT_F32, "cap_feats dtype must be bf16 or f32");
    if (lt_weights_ready(e)) return 2;
    if (refuse_profile_if_capturing(e, s, "lt_prepare_prompt")) return 2;
    const int Tpad = round_up(T, 64), cap = e->cap, A = e->A;
    ProfScope ps(e, 2, 0, s);
    if (launch_cast_to_bf16(cap_feats_dev, cap_dtype, e->capb, (long long)B * T * cap, s)) return 1;
    if (launch_mask_to_bias(cap_mask_dev, e->txt_bias, B, T, Tpad, s)) return 1;
    // adaln_input's caption half (model.py:847-850)
    if (launch_cap_pool_ln(e->capb, LT_BF16, cap_mask_dev, e->capln_w, e->capln_b, e->cap_ln, B, T, cap, s)) return 1;
    if (launch_linear_small_m(e->cap_ln, e->cape_w, e->cape_b, e->cap_emb, B, A, cap, 0, s)) return 1;
    if (prepare_caption_kv(e, B, T, Tpad, s)) return 1;
    e->prompt_B = B; e->prompt_T = T; e->prompt_Tpad = Tpad; e->reg_Y = 0;
    return 0;
}

extern "C" int lt_prepare_prompt_regional(lt_engine* e, const void* cap_feats_dev, int32_t cap_dtype, const int32_t* cap_mask_dev,
                                          int32_t Y, int32_t T, const void* global_feats_dev, const int32_t* global_mask_dev,
                                          int32_t Tg, int32_t h_split, int32_t w_split, void* stream) {
    LT_REQUIRE(e && cap_feats_dev && cap_mask_dev && global_feats_dev && global_mask_dev, "lt_prepare_prompt_regional: null argument");
    e->delta_sig[0] = 0;  // (guidance reuse: a stored difference belongs to the conditioning it was taken on)
    e->proj_sig[0] = 0;   // (projected guidance: so does a stored momentum)
    e->cache_res[0] = 0; e->cache_head[0] = 0;  // (step caching: so does a stored residual, and a probe)
    if (refuse_if_capturing((hipStream_t)stream, "lt_prepare_prompt_regional")) return 2;  // (allocates, uploads a host table, synchronises)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(e->cfg.variant == LT_VARIANT_NEXT_T2I, "lt_prepare_prompt_regional: text-conditional Next-DiT only");
    hipStream_t s = (hipStream_t)stream;
    const lt_config& c = e->cfg;
    const int Tmax = round_up(c.max_text > 0 ? c.max_text : 64, 64);
    LT_REQUIRE(Y >= 2 && Y <= c.max_batch, "%d captions exceed max_batch %d (the caption buffers are sized by it)", Y, c.max_batch);
    LT_REQUIRE(T >= 1 && T <= Tmax && Tg >= 1 && Tg <= Tmax, "text length %d / %d exceeds max_text %d", T, Tg, Tmax);
    LT_REQUIRE(h_split >= 1 && w_split >= 1, "lt_prepare_prompt_regional: split counts must be >= 1");
    LT_REQUIRE(cap_dtype == LT_BF16 || cap_dtype == LT_F32, "cap_feats dtype must be bf16 or f32");
    if (lt_weights_ready(e)) return 2;
    const int Tpad = round_up(T, 64), cap = e->cap, A = e->A;
    ProfScope ps(e, 2, 0, s);
    // adaLN conditioning from the GLOBAL caption, one row broadcast to the cond and the uncond row (model.py:866-870: the
    // pooled [1, C] embedding is added to t_emb [2, A])
    if (launch_cast_to_bf16(global_feats_dev, cap_dtype, e->capb, (long long)Tg * cap, s)) return 1;
    if (launch_cap_pool_ln(e->capb, LT_BF16, global_mask_dev, e->capln_w, e->capln_b, e->cap_ln, 1, Tg, cap, s)) return 1;
    if (launch_linear_small_m(e->cap_ln, e->cape_w, e->cape_b, e->cap_emb, 1, A, cap, 0, s)) return 1;
    LT_CHECK_HIP(hipMemcpyAsync(e->cap_emb + A, e->cap_emb, (size_t)A * 2, hipMemcpyDeviceToDevice, s));
    // the Y captions' keys / values
    if (launch_cast_to_bf16(cap_feats_dev, cap_dtype, e->capb, (long long)Y * T * cap, s)) return 1;
    if (launch_mask_to_bias(cap_mask_dev, e->txt_bias, Y, T, Tpad, s)) return 1;
    if (prepare_caption_kv(e, Y, T, Tpad, s)) return 1;
    const size_t need = (size_t)Y * c.max_tokens * e->d;
    if (e->reg_txt_elems < need) {
        // captured graphs bake this pointer into their kernels: none may outlive the buffer
        LT_CHECK_HIP(hipStreamSynchronize(s));
        for (auto& ge : e->graphs) if (ge.exec) (void)hipGraphExecDestroy(ge.exec);
        e->graphs.clear();
        if (e->reg_txt) LT_CHECK_HIP(hipFree(e->reg_txt));
        LT_CHECK_HIP(hipMalloc((void**)&e->reg_txt, need * 2));
        e->reg_txt_elems = need;
    }
    if (!e->reg_qmap) LT_CHECK_HIP(hipMalloc((void**)&e->reg_qmap, (size_t)c.max_batch * sizeof(int)));
    std::vector<int> qmap(Y, 0);
    qmap[Y - 1] = 1;
    LT_CHECK_HIP(hipMemcpyAsync(e->reg_qmap, qmap.data(), (size_t)Y * sizeof(int), hipMemcpyHostToDevice, s));
    LT_CHECK_HIP(hipStreamSynchronize(s));  // qmap is a stack temporary
    e->prompt_B = 2; e->prompt_T = T; e->prompt_Tpad = Tpad; e->reg_Y = Y; e->reg_h = h_split; e->reg_w = w_split;
    return 0;
}

extern "C" int lt_prepare_labels(lt_engine* e, const int32_t* labels_dev, int32_t B, void* stream) {
    LT_REQUIRE(e && labels_dev, "lt_prepare_labels: null argument");
    e->delta_sig[0] = 0;  // (guidance reuse: a stored difference belongs to the conditioning it was taken on)
    e->proj_sig[0] = 0;   // (projected guidance: so does a stored momentum)
    e->cache_res[0] = 0; e->cache_head[0] = 0;  // (step caching: so does a stored residual, and a probe)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(e->v.labels, "lt_prepare_labels: this variant is text-conditional (use lt_prepare_prompt)");
    LT_REQUIRE(B >= 1 && B <= e->cfg.max_batch, "label batch %d exceeds max_batch %d", B, e->cfg.max_batch);
    if (lt_weights_ready(e)) return 2;
    if (refuse_profile_if_capturing(e, (hipStream_t)stream, "lt_prepare_labels")) return 2;
    ProfScope ps(e, 2, 0, (hipStream_t)stream);
    // y_embedder(y) in eval mode (models.py:216-221) -> the label half of adaln_input (models.py:937-939)
    if (launch_label_gather(e->label_table, labels_dev, e->cap_emb, B, e->label_rows, e->A, (hipStream_t)stream)) return 1;
    e->prompt_B = B; e->prompt_T = 0; e->prompt_Tpad = 0;
    return 0;
}

extern "C" int lt_forward(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const lt_step_args* a, void* stream) {
    LT_REQUIRE(e && x_dev && t_dev && out_dev && a, "lt_forward: null argument");
    LtOptScope opt_scope(&e->opts);
    return forward_graphed(e, x_dev, t_dev, out_dev, a, 0, (hipStream_t)stream);
}

// lt_forward with the blocks of a layer set left out.  Empty set: lt_forward, capturable as it is; with a set the call is refused
// on a stream under capture (a recorded evaluation of this kind has no test behind it)
static int forward_sets(lt_engine* e, const char* who, const void* x_dev, const float* t_dev, void* out_dev, const lt_step_args* a,
                        const int32_t* skip_host, int32_t n_skip, const int32_t* perturb_host, int32_t n_perturb, void* stream) {
    LT_REQUIRE(e && x_dev && t_dev && out_dev && a, "%s: null argument", who);
    SkipScope scope(e);
    if (scope.set(who, skip_host, n_skip, perturb_host, n_perturb)) return 2;
    if ((n_skip > 0 || n_perturb > 0) && refuse_if_capturing((hipStream_t)stream, who)) return 2;
    LT_REQUIRE(n_perturb == 0 || e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): perturbed attention does not serve it", who);
    LtOptScope opt_scope(&e->opts);
    return forward_graphed(e, x_dev, t_dev, out_dev, a, 0, (hipStream_t)stream);
}

extern "C" int lt_forward_skip(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const lt_step_args* a, const int32_t* skip_host,
                               int32_t n_skip, void* stream) {
    return forward_sets(e, "lt_forward_skip", x_dev, t_dev, out_dev, a, skip_host, n_skip, nullptr, 0, stream);
}

// lt_forward with the blocks of S left out and the blocks of P perturbed.  Both sets empty: lt_forward, capturable as it is
extern "C" int lt_forward_perturb(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const lt_step_args* a, const int32_t* skip_host,
                                  int32_t n_skip, const int32_t* perturb_host, int32_t n_perturb, void* stream) {
    return forward_sets(e, "lt_forward_perturb", x_dev, t_dev, out_dev, a, skip_host, n_skip, perturb_host, n_perturb, stream);
}

// lt_forward with the blocks of S left out and the blocks of Q run on blurred queries.  Both sets empty: lt_forward, capturable as it is
extern "C" int lt_forward_blur(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const lt_step_args* a, const int32_t* skip_host,
                               int32_t n_skip, const int32_t* blur_host, int32_t n_blur, float sigma, void* stream) {
    const char* who = "lt_forward_blur";
    LT_REQUIRE(e && x_dev && t_dev && out_dev && a, "%s: null argument", who);
    if (check_blur_sets(e, who, skip_host, n_skip, blur_host, n_blur, sigma)) return 2;
    if ((n_skip > 0 || n_blur > 0) && refuse_if_capturing((hipStream_t)stream, who)) return 2;
    LT_REQUIRE(n_blur == 0 || e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): blurred queries do not serve it", who);
    if (check_blur_radius(e, who, a, n_blur, sigma)) return 2;
    if (n_blur > 0 && ensure_blur(e, sigma, (hipStream_t)stream)) return 1;
    SkipScope scope(e);
    if (scope.set_blur(who, skip_host, n_skip, blur_host, n_blur)) return 2;
    LtOptScope opt_scope(&e->opts);
    return forward_graphed(e, x_dev, t_dev, out_dev, a, 0, (hipStream_t)stream);
}

extern "C" int lt_forward_packed(lt_engine* e, const void* const* x_ptrs, const int32_t* hw_host, const float* t_dev,
                                 void* const* out_ptrs, const lt_step_args* a, void* stream) {
    LT_REQUIRE(e && x_ptrs && hw_host && t_dev && out_ptrs && a, "lt_forward_packed: null argument");
    if (refuse_if_capturing((hipStream_t)stream, "lt_forward_packed")) return 2;  // (the size table is copied from pageable host memory)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(a->batch >= 1 && a->batch <= e->cfg.max_batch, "lt_forward_packed: batch %d outside 1..max_batch %d", a->batch, e->cfg.max_batch);
    for (int b = 0; b < a->batch; ++b) LT_REQUIRE(x_ptrs[b] && out_ptrs[b], "lt_forward_packed: null sample pointer %d", b);
    if (!e->pk_dev) LT_CHECK_HIP(hipMalloc((void**)&e->pk_dev, 128 * sizeof(int)));
    PackedDesc pk{x_ptrs, out_ptrs, hw_host};
    return run_forward(e, nullptr, t_dev, nullptr, a, 0, (hipStream_t)stream, &pk);
}

// The flat form of a packed batch: the refusals of a size list, by name, before anything is launched or copied; then the device table.
int packed_call_begin(lt_engine* e, const char* who, const int32_t* hw_host, const lt_step_args* a, int use_cfg, PackedCall* pc, hipStream_t s) {
    const lt_config& c = e->cfg;
    const int B = a->batch;
    LT_REQUIRE(c.variant == LT_VARIANT_NEXT_T2I, "%s: packed batches run on the text-conditional Next-DiT (LT_VARIANT_NEXT_T2I) only; this engine is variant %d",
               who, c.variant);
    LT_REQUIRE(B >= 1 && B <= LT_PK_MAX && B <= c.max_batch, "%s: packed batch of %d samples exceeds max_batch %d (or %d)", who, B, c.max_batch, LT_PK_MAX);
    LT_REQUIRE(!use_cfg || B % 2 == 0, "%s: guidance needs an even batch (cond + uncond rows), got %d", who, B);
    LT_REQUIRE(a->io_dtype == LT_BF16 || a->io_dtype == LT_F32, "%s: io_dtype must be bf16 or f32", who);
    PackedTable t;
    int hp = 0, wp = 0;
    if (int rc = packed_table_build(hw_host, B, c.in_channels, c.patch_size, &t, &pc->elems, &pc->n_max, &hp, &wp)) return rc;
    if (use_cfg)
        for (int b = 0; b < B / 2; ++b)
            LT_REQUIRE(hw_host[2 * b] == hw_host[2 * (b + B / 2)] && hw_host[2 * b + 1] == hw_host[2 * (b + B / 2) + 1],
                       "%s: the two halves differ in size: sample %d is %dx%d, sample %d is %dx%d", who, b, hw_host[2 * b], hw_host[2 * b + 1], b + B / 2,
                       hw_host[2 * (b + B / 2)], hw_host[2 * (b + B / 2) + 1]);
    LT_REQUIRE(pc->n_max <= c.max_tokens, "%s: the longest sample has %d latent tokens, max_tokens is %d", who, pc->n_max, c.max_tokens);
    LT_REQUIRE(hp <= e->rope_len && wp <= e->rope_len, "%s: a latent grid of %dx%d tokens exceeds the RoPE table (%d)", who, hp, wp, e->rope_len);
    LT_REQUIRE(e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): regional captions take one image per call, tensor input", who);
    LT_REQUIRE(e->prompt_B == B, "%s: lt_prepare_prompt was called for batch %d, step has batch %d", who, e->prompt_B, B);
    float unused;
    if (softmax_scale_for(e, a, pc->n_max, &unused)) return 1;
    pc->hw = hw_host;
    // (the table itself travels as a kernel argument and is recordable; the first packed call of an engine allocates its device copy)
    if (!e->pk_tab && refuse_if_capturing(s, who)) return 2;
    if (!e->pk_tab) LT_CHECK_HIP(hipMalloc((void**)&e->pk_tab, sizeof(PackedTable)));
    return launch_packed_table_store(t, e->pk_tab, s);
}

extern "C" int lt_forward_cfg_packed(lt_engine* e, const void* x_flat_dev, const int32_t* hw_host, const float* t_dev, void* out_flat_dev,
                                     const lt_step_args* a, void* stream) {
    LT_REQUIRE(e && x_flat_dev && hw_host && t_dev && out_flat_dev && a, "lt_forward_cfg_packed: null argument");
    LtOptScope opt_scope(&e->opts);
    PackedCall pc{};
    if (int rc = packed_call_begin(e, "lt_forward_cfg_packed", hw_host, a, 1, &pc, (hipStream_t)stream)) return rc;
    return forward_graphed(e, x_flat_dev, t_dev, out_flat_dev, a, 1, (hipStream_t)stream, {LT_KIND_WHOLE, &pc});
}

extern "C" int lt_forward_cfg(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const lt_step_args* a, void* stream) {
    LT_REQUIRE(e && x_dev && t_dev && out_dev && a, "lt_forward_cfg: null argument");
    LtOptScope opt_scope(&e->opts);
    return forward_graphed(e, x_dev, t_dev, out_dev, a, 1, (hipStream_t)stream);
}

extern "C" int64_t lt_graph_replays(lt_engine* e) { return e ? e->graph_replays : -1; }

extern "C" int lt_set_softmax_rule(lt_engine* e, int32_t rule) {
    LT_REQUIRE(e, "lt_set_softmax_rule: null engine");
    LT_REQUIRE(e->cfg.variant == LT_VARIANT_NEXT_T2I, "lt_set_softmax_rule: the softmax rule belongs to the text-conditional Next-DiT "
               "(LT_VARIANT_NEXT_T2I) only; this engine is variant %d", e->cfg.variant);
    LT_REQUIRE(rule == LT_SOFTMAX_T2I || rule == LT_SOFTMAX_ANAGRAM, "lt_set_softmax_rule: unknown softmax rule %d (LT_SOFTMAX_T2I = 0, "
               "LT_SOFTMAX_ANAGRAM = 1)", rule);
    e->softmax_rule = rule;
    return 0;
}

// ---- MoE routing parity hooks -------------------------------------------------------------------------
namespace {
size_t moe_table_ints(const lt_engine* e) { return (size_t)e->L * 2 * e->cfg.max_batch * e->cfg.max_tokens * 2; }
}  // namespace

extern "C" int lt_moe_routing_record(lt_engine* e, int32_t on) {
    LT_REQUIRE(e && e->E > 0, "lt_moe_routing_record: not a mixture-of-experts engine");
    if (on && !e->moe_rec) {
        LT_CHECK_HIP(hipMalloc((void**)&e->moe_rec, moe_table_ints(e) * sizeof(int)));
        LT_CHECK_HIP(hipMemset(e->moe_rec, 0xff, moe_table_ints(e) * sizeof(int)));
    }
    e->moe_rec_on = on ? 1 : 0;
    return 0;
}

extern "C" int lt_moe_routing_read(lt_engine* e, int32_t* host_out, int32_t rows) {
    LT_REQUIRE(e && e->E > 0 && host_out, "lt_moe_routing_read: not a mixture-of-experts engine / null buffer");
    LT_REQUIRE(e->moe_rec && e->moe_rec_rows > 0, "lt_moe_routing_read: nothing recorded (lt_moe_routing_record, then a forward)");
    LT_REQUIRE(rows == e->moe_rec_rows, "lt_moe_routing_read: the last recorded call had %d rows, not %d", e->moe_rec_rows, rows);
    LT_CHECK_HIP(hipDeviceSynchronize());
    const size_t cap = (size_t)e->cfg.max_batch * e->cfg.max_tokens * 2;
    for (int lb = 0; lb < e->L * 2; ++lb)
        LT_CHECK_HIP(hipMemcpy(host_out + (size_t)lb * rows * 2, e->moe_rec + (size_t)lb * cap, (size_t)rows * 2 * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lt_moe_routing_force(lt_engine* e, const int32_t* host_sel, int32_t rows) {
    LT_REQUIRE(e && e->E > 0, "lt_moe_routing_force: not a mixture-of-experts engine");
    if (!host_sel || rows <= 0) { e->moe_force_rows = 0; return 0; }
    LT_REQUIRE((long long)rows <= (long long)e->cfg.max_batch * e->cfg.max_tokens, "lt_moe_routing_force: %d rows exceed the engine's capacity", rows);
    // per (layer, branch): a branch this variant RUNS needs two distinct expert ids in 0..E-1 for every row (a -1 there reached
    // the plan kernel's packed counters as a negative shift and corrupted the plan silently - ADVICE r3); a branch it does not run
    // (moe_mode 1: space, 2: time) may carry anything, -1 by convention, and is never read
    for (int lb = 0; lb < e->L * 2; ++lb) {
        const int branch = lb & 1;
        const bool runs = e->moe_mode == 0 || (e->moe_mode == 1 && branch == 0) || (e->moe_mode == 2 && branch == 1);
        const int32_t* tb = host_sel + (size_t)lb * rows * 2;
        for (int r = 0; r < rows; ++r) {
            const int a = tb[2 * r], b = tb[2 * r + 1];
            if (!runs) {
                LT_REQUIRE(a >= -1 && a < e->E && b >= -1 && b < e->E, "lt_moe_routing_force: expert id outside -1..%d (layer %d, branch %d, row %d)", e->E - 1, lb >> 1, branch, r);
                continue;
            }
            LT_REQUIRE(a >= 0 && a < e->E && b >= 0 && b < e->E, "lt_moe_routing_force: layer %d branch %d row %d: expert ids (%d, %d) must lie in 0..%d (this branch runs)",
                       lb >> 1, branch, r, a, b, e->E - 1);
            LT_REQUIRE(a != b, "lt_moe_routing_force: layer %d branch %d row %d selects expert %d twice (top-2 picks two different experts)", lb >> 1, branch, r, a);
        }
    }
    if (!e->moe_force) LT_CHECK_HIP(hipMalloc((void**)&e->moe_force, moe_table_ints(e) * sizeof(int)));
    LT_CHECK_HIP(hipDeviceSynchronize());
    const size_t cap = (size_t)e->cfg.max_batch * e->cfg.max_tokens * 2;
    for (int lb = 0; lb < e->L * 2; ++lb)
        LT_CHECK_HIP(hipMemcpy(e->moe_force + (size_t)lb * cap, host_sel + (size_t)lb * rows * 2, (size_t)rows * 2 * sizeof(int), hipMemcpyHostToDevice));
    e->moe_force_rows = rows;
    return 0;
}

// ---- profiling ------------------------------------------------------------------------------------------
extern "C" int lt_profile_enable(lt_engine* e, int32_t on) {
    LT_REQUIRE(e, "null engine");
    // under rocprofv3 the tool intercepts every event / signal; tens of thousands of warm-up records crash it (ROCm 7.2), and
    // its own kernel trace is what such a run is for: LT_NO_EVENT_PROFILE=1 (scripts/gpu_prof.sh) turns the engine's events off
    if (on && getenv("LT_NO_EVENT_PROFILE")) { e->prof_on = false; e->prof_mask = 0; return 0; }
    if (on) {
        const size_t want[3] = {2048, 512, 2048};  // launches bracketed per class before read-out scales up (lt_profile_read)
        bool created = false;
        for (int k = 0; k < 3; ++k) {
            while (e->prof[k].ev.size() < want[k]) {
                hipEvent_t a, b;
                // device-scope release: the default event flags make every record a system-scope release (L2 write-back)
                LT_CHECK_HIP(hipEventCreateWithFlags(&a, hipEventReleaseToDevice));
                LT_CHECK_HIP(hipEventCreateWithFlags(&b, hipEventReleaseToDevice));
                e->prof[k].ev.push_back({a, b});
                created = true;
            }
        }
        if (created) {  // first use of an event allocates its signal (tens of us): pay that here, not in a timed region
            for (int k = 0; k < 3; ++k)
                for (auto& pr : e->prof[k].ev) {
                    LT_CHECK_HIP(hipEventRecord(pr.first, nullptr));
                    LT_CHECK_HIP(hipEventRecord(pr.second, nullptr));
                }
            LT_CHECK_HIP(hipStreamSynchronize(nullptr));
        }
    }
    e->prof_on = on != 0;
    e->prof_mask = on == 1 ? 7 : (on & 7);  // 1 = all classes (historic), otherwise bit mask: 1 GEMM | 2 attention | 4 other
    return 0;
}

extern "C" int lt_profile_enable_mask(lt_engine* e, int32_t mask) {
    LT_REQUIRE(e && mask >= 0 && mask <= 7, "lt_profile_enable_mask: mask 0..7");
    if (lt_profile_enable(e, mask ? 7 : 0)) return 1;  // event pools; honours LT_NO_EVENT_PROFILE
    if (e->prof_on) e->prof_mask = mask;
    return 0;
}

extern "C" int lt_profile_set_budget(lt_engine* e, int32_t klass, int64_t max_event_launches) {
    LT_REQUIRE(e && klass >= 0 && klass < 3, "lt_profile_set_budget: bad class");
    e->prof[klass].budget = max_event_launches < 0 ? (size_t)-1 : (size_t)max_event_launches;
    e->prof[klass].skip = 0;
    return 0;
}

extern "C" int lt_profile_set_window(lt_engine* e, int32_t klass, int64_t skip_launches, int64_t max_event_launches) {
    LT_REQUIRE(e && klass >= 0 && klass < 3 && skip_launches >= 0, "lt_profile_set_window: bad arguments");
    e->prof[klass].skip = skip_launches;
    e->prof[klass].budget = max_event_launches < 0 ? (size_t)-1 : (size_t)max_event_launches;
    return 0;
}

extern "C" int lt_profile_reset(lt_engine* e) {
    LT_REQUIRE(e, "null engine");
    for (int k = 0; k < 3; ++k) { e->prof[k].flops = 0; e->prof[k].launches = 0; e->prof[k].used = 0; }
    return 0;
}

extern "C" int lt_profile_read(lt_engine* e, int32_t klass, double* ms, int64_t* launches, double* flops) {
    LT_REQUIRE(e && klass >= 0 && klass < 3, "lt_profile_read: bad class");
    ProfClass& pc = e->prof[klass];
    double total = 0;
    for (size_t i = 0; i < pc.used; ++i) {
        float t = 0;
        LT_CHECK_HIP(hipEventElapsedTime(&t, pc.ev[i].first, pc.ev[i].second));
        total += t;
    }
    // scale to all launches of the class if the event pool ran out (same launch mix every step)
    if (pc.used > 0 && (long long)pc.used < pc.launches) total *= (double)pc.launches / (double)pc.used;
    if (ms) *ms = total;
    if (launches) *launches = pc.launches;
    if (flops) *flops = pc.flops;
    return 0;
}

// Options (options.h).  lt_set_option: the process default - what every engine without its own override, and every lt_op_* operator
// call, sees.  lt_engine_set_option: an override for one engine (value LT_OPTION_INHERIT drops it again); it applies to every later call
// on that engine, from any thread, and to nothing else.  Both validate against the option table (gemm_prefetch, gemm_splitk
// and gemm_w4q_grouped used to accept any integer).
// returns the option's index, -1 for a retired name given its only accepted value (nothing to do), -2 after lt_set_error
static int option_lookup(const char* name, int32_t* value, const char* who) {
    if (!name) { lt_set_error("%s: null name", who); return -2; }
    if (strcmp(name, "gemm_pipeline") == 0 || strcmp(name, "gemm_pp_tail") == 0 || strcmp(name, "gemm_persist") == 0) {
        // round-1 study knobs: the kernels they selected were deleted with csrc/experimental/ in round 5
        if (*value != 0) { lt_set_error("%s(%s): removed - the round-1 study kernels are gone (git history keeps them)", who, name); return -2; }
        return -1;
    }
    const int id = lt_opt_find(name);
    if (id < 0) {
        lt_set_error("%s: unknown option '%s'", who, name);
        return -2;
    }
    int v = *value;
    if (lt_opt_validate(id, &v)) return -2;
    *value = v;
    return id;
}

extern "C" int lt_set_option(const char* name, int32_t value) {
    const int id = option_lookup(name, &value, "lt_set_option");
    if (id == -2) return 2;
    if (id >= 0) lt_opt_set_process(id, value);
    return 0;
}

extern "C" int lt_engine_set_option(lt_engine* e, const char* name, int32_t value) {
    LT_REQUIRE(e, "lt_engine_set_option: null engine");
    const bool inherit = value == LT_OPTION_INHERIT;
    int32_t v = inherit ? 0 : value;
    int id;
    if (inherit) {
        id = lt_opt_find(name);
        LT_REQUIRE(id >= 0, "lt_engine_set_option: unknown option '%s'", name ? name : "(null)");
    } else {
        id = option_lookup(name, &v, "lt_engine_set_option");
        if (id == -2) return 2;
        if (id < 0) return 0;
    }
    e->opts.v[id].store(inherit ? LT_OPT_INHERIT : v, std::memory_order_relaxed);
    e->opts.gen.fetch_add(1, std::memory_order_release);  // new HIP-graph keys: kernel selection is baked into a captured graph
    return 0;
}

extern "C" int lt_engine_get_option(lt_engine* e, const char* name, int32_t* value) {
    LT_REQUIRE(name && value, "lt_engine_get_option: null argument");
    if (strcmp(name, "last_pair") == 0) {  // read-only, no option: the operand layout regime of the engine's last evaluation (lumina_dit_debug.h)
        LT_REQUIRE(e, "lt_engine_get_option: last_pair: null engine");
        *value = e->last_pair ? 1 : 0;
        return 0;
    }
    if (strcmp(name, "layout_flips") == 0) {  // read-only, no option: weight layout conversions during the last sampler call (lumina_dit_debug.h)
        LT_REQUIRE(e, "lt_engine_get_option: layout_flips: null engine");
        *value = (int32_t)std::min<long long>(e->layout_flips, INT32_MAX);
        return 0;
    }
    if (strcmp(name, "layout_pinned") == 0) {  // read-only, no option: a caller's graph holds an evaluation, the weights stay row-major (lumina_dit_debug.h)
        LT_REQUIRE(e, "lt_engine_get_option: layout_pinned: null engine");
        *value = e->layout_pinned ? 1 : 0;
        return 0;
    }
    const int id = lt_opt_find(name);
    LT_REQUIRE(id >= 0, "lt_engine_get_option: unknown option '%s'", name);
    LtOptScope opt_scope(e ? &e->opts : nullptr);  // e == NULL: the process default
    *value = lt_opt(id);
    return 0;
}
