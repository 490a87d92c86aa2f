// Whole-trajectory samplers of the C ABI (include/lumina_dit.h): the fixed-grid ODE loop of transport/integrators.py:104-116 (torchdiffeq
// euler / midpoint / rk4; with an inpainting mask; with a guidance scale per stage), multi-view (visual-anagram) sampling, the SDE loop and the
// adaptive Runge-Kutta loop.  One call per trajectory, no
// host<->device sync inside it (the adaptive loop reads one error ratio per attempted step).  All
// are written against one scaffold - check_step_shape, StageTimes (engine.h), Trajectory, GuidancePlan (guidance_plan.h) - and a new sampler is too: what a sampler
// owns is its stage-time fill loop and its stepping body, where the reference's rounding points are.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "engine.h"
#include "guidance_plan.h"
#include "kernels.h"

namespace {

// the state buffers were sized by lt_create for max_batch x max_tokens; checked before the first copy into them (the model calls validate
// the same things, but only after z has been copied)
int check_latent(const lt_engine* e, const char* who, int h, int w) {
    const int p = e->cfg.patch_size;
    LT_REQUIRE(h > 0 && w > 0 && h % p == 0 && w % p == 0 && (long long)(h / p) * (w / p) <= e->cfg.max_tokens,
               "%s: latent %dx%d is not a positive multiple of the patch size or exceeds max_tokens %d", who, h, w, e->cfg.max_tokens);
    return 0;
}

int check_step_shape(const lt_engine* e, const char* who, const lt_step_args* a) {
    LT_REQUIRE(a->batch >= 1 && a->batch <= e->cfg.max_batch, "%s: batch %d outside 1..max_batch %d", who, a->batch, e->cfg.max_batch);
    if (check_latent(e, who, a->latent_h, a->latent_w)) return 2;
    LT_REQUIRE(a->io_dtype == LT_BF16 || a->io_dtype == LT_F32, "io_dtype must be bf16 or f32");
    return 0;
}

// masked sampling refuses the multistep methods by name, in front of the method range
int refuse_masked_multistep(const char* who, int method) {
    LT_REQUIRE(!(method >= LT_ODE_AB2 && method <= LT_ODE_ABM3), "%s: masked sampling with a multistep method (ab2, ab3, abm2, abm3) is refused: the blend "
               "makes the state discontinuous, so the history's slopes no longer belong to it", who);
    return 0;
}
// the grid and the method of a fixed-grid call, in this order; `note`: what the call adds to the method's refusal
int check_grid_method(const char* who, int n_grid, int method, bool masked, const char* note) {
    LT_REQUIRE(n_grid >= 2, "%s: need at least 2 grid points", who);
    if (masked && refuse_masked_multistep(who, method)) return 2;
    LT_REQUIRE(method >= LT_ODE_EULER && method <= LT_ODE_RK4, "%s: unknown method %d%s", who, method, note);
    return 0;
}

// ---- the buffers an evaluation stores for a later one (LtStoredBuffer, guidance_plan.h): the cond - uncond difference e->g_delta,
// APG's momentum e->p_mom (7q), the block stack's residual e->c_r (7n).  Each has a signature in the engine, and one protocol, written here once
int* stored_sig(lt_engine* e, LtStoredBuffer buf) {
    return buf == LT_STORED_DELTA ? e->delta_sig : buf == LT_STORED_MOMENTUM ? e->proj_sig : buf == LT_STORED_RESIDUAL ? e->cache_res : nullptr;
}
// what the buffer holds after an evaluation of these step arguments that rewrites it: the difference and the momentum { B', H, W, ch } of the
// guided channels, the residual { B, H, W, use_cfg }
void stored_sig_of(const lt_engine* e, LtStoredBuffer buf, const lt_step_args* a, int use_cfg, int sig[4]) {
    const int cfg_ch = a->cfg_channels > 0 ? a->cfg_channels : 3;
    const bool res = buf == LT_STORED_RESIDUAL;
    sig[0] = res ? a->batch : a->batch / 2; sig[1] = a->latent_h; sig[2] = a->latent_w;
    sig[3] = res ? (use_cfg ? 1 : 0) : std::min(cfg_ch, (int)e->cfg.in_channels);
}
bool same_sig(const int have[4], const int want[4]) { return have[0] == want[0] && have[1] == want[1] && have[2] == want[2] && have[3] == want[3]; }
// one evaluation that rewrites `buf` (LT_STORED_NONE: none): the signature is forgotten until the evaluation has been issued whole
int forward_rewriting(lt_engine* e, LtStoredBuffer buf, const void* x, const float* t, void* out, const lt_step_args* a, int use_cfg, hipStream_t s,
                      const EvalSpec& spec) {
    int* sig = stored_sig(e, buf);
    if (sig) sig[0] = 0;
    if (int rc = forward_graphed(e, x, t, out, a, use_cfg, s, spec)) return rc;
    if (sig) stored_sig_of(e, buf, a, use_cfg, sig);
    return 0;
}
// a call that continues from the stored difference or momentum: refused by name unless the buffer holds one of this call's shape
int check_stored(lt_engine* e, const char* who, LtStoredBuffer buf, const lt_step_args* a, const char* what, const char* use, const char* absent) {
    int want[4];
    stored_sig_of(e, buf, a, 1, want);
    const int* have = stored_sig(e, buf);
    LT_REQUIRE(have[0] != 0, "%s: no stored %s to %s: %s, or lt_prepare_prompt / lt_prepare_labels was called since", who, what, use, absent);
    LT_REQUIRE(same_sig(have, want), "%s: the stored %s is of another shape: %d samples of %d channels at %dx%d, the call has %d samples of %d "
               "channels at %dx%d", who, what, have[0], have[3], have[1], have[2], want[0], want[3], want[1], want[2]);
    return 0;
}
// APG's momentum starts at zero: every trajectory, and a single evaluation that does not continue
int zero_momentum(lt_engine* e, const lt_step_args* a, hipStream_t s) {
    int sig[4];
    stored_sig_of(e, LT_STORED_MOMENTUM, a, 1, sig);
    e->proj_sig[0] = 0;
    LT_CHECK_HIP(hipMemsetAsync(e->p_mom, 0, (size_t)sig[0] * sig[3] * sig[1] * sig[2] * sizeof(float), s));
    return 0;
}
// the head of a step-cached evaluation and its two indicator sums in e->c_sums_host: one synchronisation
int cache_probe(lt_engine* e, const void* x, const float* t, const lt_step_args* a, int use_cfg, hipStream_t s) {
    if (int rc = forward_graphed(e, x, t, nullptr, a, use_cfg, s, {LT_KIND_CACHE_HEAD})) return rc;
    LT_CHECK_HIP(hipMemcpyAsync(e->c_sums_host, e->c_ws + 2 * LT_CACHE_BLOCKS, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    LT_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}
// A stage of skip-layer guidance with s != 0: the cond rows with the blocks of `sets` left out / perturbed, their guided
// channels kept; then the stage's own evaluation `closing` - all rows, or the cond rows at scale 1 - whose closing kernel adds s (cond - skip).
// s_dev: where s is, to be put into its fixed word between the two; null: it is in place
int forward_slg_pair(lt_engine* e, const char* who, const GuidancePlan& sets, const void* x, const float* t, void* out, const lt_step_args* a,
                     hipStream_t s, LtEvalKind closing, const float* closing_scale, const float* s_dev) {
    {
        SkipScope scope(e);
        if (sets.n_blur > 0 ? scope.set_blur(who, sets.skip, sets.n_skip, sets.blur, sets.n_blur)  // (the entry point has run ensure_blur)
                            : scope.set(who, sets.skip, sets.n_skip, sets.perturb, sets.n_perturb)) return 2;
        if (int rc = forward_graphed(e, x, t, nullptr, a, 1, s, {LT_KIND_SLG_STORE, nullptr, e->g_cfg})) return rc;
    }
    if (s_dev) LT_CHECK_HIP(hipMemcpyAsync(e->g_cfg + 3, s_dev, sizeof(float), hipMemcpyDeviceToDevice, s));
    return forward_graphed(e, x, t, out, a, 1, s, {closing, nullptr, closing_scale});
}

// The state of one trajectory: the ping-pong pair e->ys, the caller's record of the states (if any), the evaluation and row counts, and the
// plan (guidance_plan.h) that says what evaluation number `call` issues - the empty plan: every one whole.
struct Trajectory {
    lt_engine* e; const lt_step_args* a; int use_cfg; hipStream_t s;
    size_t sbytes;  // one state
    const PackedCall* pc = nullptr;  // a packed batch: the states are flat buffers (lt_sample_ode_packed)
    GuidancePlan plan;
    int ncalls = 0;  // the evaluations of the committed table: the plan's tail lies behind their stage times
    void* traj = nullptr;
    int cur = 0;
    long long nfe = 0, rows = 0, flips0 = 0, hits = 0;  // hits: the step-cached evaluations that reused the residual
    int start(const void* z, void* traj_dev, bool z_in_slot0) {
        traj = traj_dev;
        flips0 = e->layout_flips_total;
        LT_CHECK_HIP(hipMemcpyAsync(e->ys[0], z, sbytes, hipMemcpyDeviceToDevice, s));
        if (traj && z_in_slot0) LT_CHECK_HIP(hipMemcpyAsync(traj, z, sbytes, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    void* y0() const { return e->ys[cur]; }      // the current state
    void* y1() const { return e->ys[cur ^ 1]; }  // where the step writes the next one
    // one model evaluation at stage time number `call` of the committed table: the plan's step, its evaluations and rows counted
    int eval(const void* y, int call, void* out) {
        ++nfe;
        const float* t = e->times.dev + (size_t)call * a->batch;
        const GuidanceStep st = plan.step_of(call);
        if (st.kinds[0] == LT_KIND_CACHE_HEAD) return eval_cached(y, t, call, out);
        const float* scale = st.scale == LT_SCALE_TABLE ? e->times.dev + GuidancePlan::table_offset(ncalls, a->batch) + call
                             : st.scale == LT_SCALE_FIXED ? e->g_cfg : nullptr;
        for (int k = 0; k < st.n_kinds; ++k) rows += lt_eval_traits(st.kinds[k]).half ? a->batch / 2 : a->batch;
        if (st.n_kinds == 2) {  // (the sets were checked by the entry point)
            ++nfe;
            return forward_slg_pair(e, "skip-layer guidance", plan, y, t, out, a, s, st.kinds[1], scale,
                                    e->times.dev + GuidancePlan::second_offset(ncalls, a->batch) + call);
        }
        return forward_rewriting(e, st.rewrites, y, t, out, a, lt_eval_traits(st.kinds[0]).dev_scale ? 1 : use_cfg, s, {st.kinds[0], pc, scale});
    }
    // an evaluation under step caching: the head, the two indicator sums to the host (the first and the last evaluation run the stack
    // whatever they are and read nothing), the controller, then the stack + tail or the stored residual + tail
    int eval_cached(const void* y, const float* t, int call, void* out) {
        CacheControl* cache = plan.cache;
        bool run = true;
        double rel = 0.0;
        if (call > 0 && call < ncalls - 1) {
            if (int rc = cache_probe(e, y, t, a, use_cfg, s)) return rc;
            run = cache->step(e->c_sums_host[0], e->c_sums_host[1], &rel);
        } else if (int rc = forward_graphed(e, y, t, nullptr, a, use_cfg, s, {LT_KIND_CACHE_HEAD})) {
            return rc;
        }
        if (cache->stats) { cache->stats[3 * call] = rel; cache->stats[3 * call + 1] = cache->acc; cache->stats[3 * call + 2] = run ? 1.0 : 0.0; }
        if (!run) {
            ++hits;
            return forward_graphed(e, y, t, out, a, use_cfg, s, {LT_KIND_CACHE_APPLY});
        }
        cache->acc = 0.0;
        rows += a->batch;  // (the head and the blocks are one evaluation; a reuse counts no rows)
        return forward_rewriting(e, LT_STORED_RESIDUAL, y, t, out, a, use_cfg, s, {LT_KIND_CACHE_BLOCKS});
    }
    int advance(int traj_slot) {  // y1 is the current state now [and slot `traj_slot` of the record]
        if (traj) LT_CHECK_HIP(hipMemcpyAsync((char*)traj + (size_t)traj_slot * sbytes, y1(), sbytes, hipMemcpyDeviceToDevice, s));
        cur ^= 1;
        return 0;
    }
    int finish(void* final_dev) {  // (null: not asked for, or the last step's kernel wrote it)
        if (final_dev) LT_CHECK_HIP(hipMemcpyAsync(final_dev, y0(), sbytes, hipMemcpyDeviceToDevice, s));
        e->last_nfe = nfe;
        e->last_eval_rows = rows;
        if (plan.form == LT_PLAN_CACHED) e->last_cache_hits = hits;
        e->layout_flips = e->layout_flips_total - flips0;
        return 0;
    }
};

float bf16_round_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    u &= 0xffff0000u;
    memcpy(&f, &u, 4);
    return f;
}

// One call of a grid loop: the states, the grid, the stepping rule - `method` (ode_fixed_grid) or the weight table and `corrector`
// (ode_multistep) - and the state's n elements (the stage arithmetic is elementwise, so a packed batch's flat state, `pc`, runs as it is)
struct GridCall {
    const void* z; void *traj, *final;
    const float* tgrid; int n_grid, use_cfg, t_round;
    const lt_step_args* a; hipStream_t s; long long n; const PackedCall* pc;
    int method = 0; const float* coef = nullptr; int corrector = 0;
    bool tiled = false;  // lt_sample_ode_tiled: the state is the canvas, an evaluation is e->tw's windows gathered, evaluated and fused
    // lt_sample_ode_compose (compose_K > 0): the state has a->batch / (K + 1) rows, an evaluation is the state replicated under the K + 1 prompts,
    // evaluated and composed with row `call` of the [ncalls][K] weight table
    int compose_K = 0; const float* compose_w = nullptr;
};
struct MaskedBlend { const void *mask, *x1, *noise; };

// the state of a dense batch, in elements
long long dense_elems(const lt_engine* e, const lt_step_args* a) { return (long long)a->batch * e->cfg.in_channels * a->latent_h * a->latent_w; }

// What a plan puts on the device once, behind the commit of its tail: the rule pair into e->g_cfg[1..2]; eta, beta, r into their fixed words,
// and APG's momentum starts every trajectory at zero
int apply_plan(lt_engine* e, const GuidancePlan& plan, const lt_step_args* a, int ncalls, hipStream_t s) {
    const float* second = e->times.dev + GuidancePlan::second_offset(ncalls, a->batch);
    if (plan.projected()) LT_CHECK_HIP(hipMemcpyAsync(e->p_par + 1, second, 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (plan.form == LT_PLAN_PROJECT_APG && zero_momentum(e, a, s)) return 1;
    if (plan.form == LT_PLAN_RULE) LT_CHECK_HIP(hipMemcpyAsync(e->g_cfg + 1, second, 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

// The fixed-grid loop: stage-time fill and the euler / midpoint / rk4 stepping body.  The callers have validated the grid, the method and the
// shape.  With `mb` (lt_sample_ode_masked; null: none) the LAST combine of every step is the masked launcher - the same arithmetic followed by
// the inpainting blend at the step's end time - and nothing else changes.  Evaluation i * stages + k is what the plan says: its tables are
// committed behind the stage times (GuidancePlan: the tail) and its fixed parameters put in place once (apply_plan).
int ode_fixed_grid(lt_engine* e, const GridCall& c, const GuidancePlan& plan, const MaskedBlend* mb) {
    const lt_step_args* a = c.a;
    hipStream_t s = c.s;
    const float* tgrid_host = c.tgrid;
    const int B = a->batch, n_grid = c.n_grid, method = c.method;
    const long long n = c.n;
    const int stages = method == LT_ODE_EULER ? 1 : (method == LT_ODE_MIDPOINT ? 2 : 4);
    const int ncalls = (n_grid - 1) * stages;
    const bool bf = a->io_dtype == LT_BF16;
    // stage times; torchdiffeq's _PerturbFunc casts t to the state dtype before calling the model, then
    // integrators.py:108 broadcasts it to an fp32 [B] vector
    const int nsent = ncalls * B + plan.tail_floats(ncalls);
    float* tp = e->times.begin(nsent, s);
    if (!tp) return 1;
    std::vector<float> dts(n_grid - 1);
    for (int i = 0; i + 1 < n_grid; ++i) {
        const float t0 = tgrid_host[i], t1 = tgrid_host[i + 1];
        const float dt = t1 - t0;
        dts[i] = dt;
        float ts[4];
        if (method == LT_ODE_EULER) ts[0] = t0;
        else if (method == LT_ODE_MIDPOINT) { ts[0] = t0; ts[1] = t0 + 0.5f * dt; }
        else { ts[0] = t0; ts[1] = t0 + dt * (float)(1.0 / 3.0); ts[2] = t0 + dt * (float)(2.0 / 3.0); ts[3] = t1; }
        for (int k = 0; k < stages; ++k) {
            const float tv = (c.t_round && bf) ? bf16_round_host(ts[k]) : ts[k];
            for (int b = 0; b < B; ++b) tp[((size_t)i * stages + k) * B + b] = tv;
        }
    }
    plan.fill_tail(tp + GuidancePlan::table_offset(ncalls, B), ncalls);
    if (e->times.commit(nsent, s) || apply_plan(e, plan, a, ncalls, s)) return 1;
    Trajectory tr{e, a, c.use_cfg, s, (size_t)n * (bf ? 2 : 4), c.pc, plan, ncalls};
    if (tr.start(c.z, c.traj, true)) return 1;
    const int dt_code = bf ? 1 : 0;
    // one velocity of the state: the model on it, or (tiled) on its windows, whose predictions are fused into `out`, or (composed,
    // DESIGN 7s) on its copies under K + 1 prompts, whose predictions are composed into `out`
    auto eval = [&](const void* y, int call, void* out) -> int {
        if (c.compose_K) {  // 
            const int K = c.compose_K, Bp = B / (K + 1), C = e->cfg.in_channels, HW = a->latent_h * a->latent_w;
            if (launch_compose_replicate(y, e->tw_in, K, Bp, C, HW, dt_code, s)) return 1;
            if (tr.eval(e->tw_in, call, e->tw_out)) return 1;
            return launch_compose_guidance(e->tw_out, out, c.compose_w + (size_t)call * K, K, Bp, C, HW, a->cfg_channels, dt_code, s);
        }
        if (!c.tiled) return tr.eval(y, call, out);
        if (launch_windows_gather(y, e->tw, e->tw_in, e->cfg.in_channels, dt_code, s)) return 1;
        if (tr.eval(e->tw_in, call, e->tw_out)) return 1;
        return launch_windows_reduce(e->tw_out, e->tw, e->tw_has_weight ? e->tw_weight : nullptr, e->tw_wsum, out, e->cfg.in_channels, dt_code, s);
    };
    for (int i = 0; i + 1 < n_grid; ++i) {
        void *y0 = tr.y0(), *y1 = tr.y1();
        if (i < plan.zero_init) {  // CFG-Zero*'s zero-init: zero velocity, so the state stays where it is; no evaluation, nothing counted
            if (tr.traj) LT_CHECK_HIP(hipMemcpyAsync((char*)tr.traj + (size_t)(i + 1) * tr.sbytes, y0, tr.sbytes, hipMemcpyDeviceToDevice, s));
            continue;
        }
        // torchdiffeq multiplies the 0-dim DEVICE tensor dt = t1 - t0 (fp32) with the bf16 state / slopes; PyTorch's type
        // promotion keeps bf16 and casts the 0-dim operand to it first, so with a bf16 state every `dt * k` of the reference
        // sees bf16(dt) (0.5 dt is exact after that).  The stage TIMES above stay fp32 (t0 + dt / 2 is fp32 arithmetic).
        const float dt = bf ? bf16_round_host(dts[i]) : dts[i];
        const int c0 = i * stages;
        // the step's closing combine: y1 = y0 + ... [then blended with the known path at t1: the host loop's Python floats t1 and 1 - t1, the
        // latter formed in double, enter torch's fp32 op-math]
        auto close = [&](int mode, const void* k1, const void* k2, const void* k3, const void* k4) -> int {
            if (!mb) return launch_ode_combine(mode, y0, k1, k2, k3, k4, y1, dt_code, dt, n, s);
            const float t1 = tgrid_host[i + 1];
            return launch_ode_combine_masked(mode, y0, k1, k2, k3, k4, mb->mask, mb->x1, mb->noise, y1, dt_code, dt, t1, (float)(1.0 - (double)t1), n, s);
        };
        if (method == LT_ODE_EULER) {
            if (eval(y0, c0, e->kbuf[0])) return 1;
            if (close(0, e->kbuf[0], nullptr, nullptr, nullptr)) return 1;
        } else if (method == LT_ODE_MIDPOINT) {
            if (eval(y0, c0, e->kbuf[0])) return 1;
            if (launch_ode_combine(0, y0, e->kbuf[0], nullptr, nullptr, nullptr, e->ymid, dt_code, 0.5f * dt, n, s)) return 1;
            if (eval(e->ymid, c0 + 1, e->kbuf[1])) return 1;
            if (close(0, e->kbuf[1], nullptr, nullptr, nullptr)) return 1;
        } else {
            if (eval(y0, c0, e->kbuf[0])) return 1;
            if (launch_ode_combine(1, y0, e->kbuf[0], nullptr, nullptr, nullptr, e->ymid, dt_code, dt, n, s)) return 1;
            if (eval(e->ymid, c0 + 1, e->kbuf[1])) return 1;
            if (launch_ode_combine(2, y0, e->kbuf[0], e->kbuf[1], nullptr, nullptr, e->ymid, dt_code, dt, n, s)) return 1;
            if (eval(e->ymid, c0 + 2, e->kbuf[2])) return 1;
            if (launch_ode_combine(3, y0, e->kbuf[0], e->kbuf[1], e->kbuf[2], nullptr, e->ymid, dt_code, dt, n, s)) return 1;
            if (eval(e->ymid, c0 + 3, e->kbuf[3])) return 1;
            if (close(4, e->kbuf[0], e->kbuf[1], e->kbuf[2], e->kbuf[3])) return 1;
        }
        if (tr.advance(i + 1)) return 1;
    }
    return tr.finish(c.final);
}

}  // namespace

// lt_sample_ode and its packed (`hw_host`; null: a dense batch) and masked (`mb`; null: no blend) forms, which differ in what they check
static int sample_plain(lt_engine* e, const char* who, GridCall c, const int32_t* hw_host, bool packed, const MaskedBlend* mb) {
    // (the mask pointers before e: the tests pin the first error)
    LT_REQUIRE(!mb || (mb->mask && mb->x1 && mb->noise), "%s: null mask, source or noise", who);
    LT_REQUIRE(e && c.z && c.tgrid && c.a && (hw_host || !packed), "%s: null argument", who);
    if (refuse_if_capturing(c.s, who)) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    if (check_grid_method(who, c.n_grid, c.method, mb != nullptr, "")) return 2;
    PackedCall pc{};
    if (packed) {
        if (int rc = packed_call_begin(e, who, hw_host, c.a, c.use_cfg, &pc, c.s)) return rc;
        c.n = pc.elems; c.pc = &pc;
    } else {
        if (check_step_shape(e, who, c.a)) return 2;
        // (lt_sample_ode leaves this to the first evaluation, after z has been copied; a masked call writes nothing)
        LT_REQUIRE(!mb || !c.use_cfg || c.a->batch % 2 == 0, "%s: guidance needs an even batch (cond + uncond rows), got %d", who, c.a->batch);
        c.n = dense_elems(e, c.a);
    }
    return ode_fixed_grid(e, c, {}, mb);
}

extern "C" int lt_sample_ode(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host,
                             int32_t n_grid, int32_t method, int32_t use_cfg, int32_t t_round, const lt_step_args* a,
                             void* stream) {
    return sample_plain(e, "lt_sample_ode", {z_dev, traj_dev, final_dev, tgrid_host, n_grid, use_cfg, t_round, a, (hipStream_t)stream, 0, nullptr, method}, nullptr,
                        false, nullptr);
}

// Step caching: what the cached entry points refuse beyond lt_sample_ode's refusals, by name, before anything is launched
static int check_cached_call(lt_engine* e, const char* who, const lt_step_args* a, int use_cfg) {
    if (check_step_shape(e, who, a)) return 2;
    LT_REQUIRE(!use_cfg || a->batch % 2 == 0, "%s: guidance needs an even batch (cond + uncond rows), got %d", who, a->batch);
    LT_REQUIRE(e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): step caching does not serve it", who);
    LT_REQUIRE(!e->moe_rec_on && !e->moe_force_rows, "%s: MoE routing record / force is on: step caching does not serve it", who);
    LT_REQUIRE(e->skip.empty(), "%s: a layer-skip set is not served", who);
    LT_REQUIRE(e->prompt_B == a->batch, "%s: %s was called for batch %d, step has batch %d", who, e->v.labels ? "lt_prepare_labels" : "lt_prepare_prompt",
               e->prompt_B, a->batch);
    return 0;
}

extern "C" int lt_sample_ode_cached(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                    int32_t method, int32_t use_cfg, int32_t t_round, const lt_step_args* a, float threshold,
                                    const double* coef_host, double* stats_host, void* stream) {
    LT_REQUIRE(e && z_dev && tgrid_host && a && coef_host, "lt_sample_ode_cached: null argument");
    if (refuse_if_capturing((hipStream_t)stream, "lt_sample_ode_cached")) return 2;  // (the controller reads the indicator on the host)
    LtOptScope opt_scope(&e->opts);
    if (check_grid_method("lt_sample_ode_cached", n_grid, method, false, " (step caching serves the fixed-grid methods euler, midpoint, rk4; not the "
                          "multistep and adaptive solvers)")) return 2;
    LT_REQUIRE(threshold >= 0.0f, "lt_sample_ode_cached: threshold %g is not a number >= 0", (double)threshold);
    for (int k = 0; k < 5; ++k) LT_REQUIRE(std::isfinite(coef_host[k]), "lt_sample_ode_cached: coefficient %d is not finite", k);
    if (check_cached_call(e, "lt_sample_ode_cached", a, use_cfg)) return 2;
    if (ensure_step_cache(e)) return 1;
    CacheControl cc{(double)threshold, {coef_host[0], coef_host[1], coef_host[2], coef_host[3], coef_host[4]}, 0.0, stats_host};
    return ode_fixed_grid(e, {z_dev, traj_dev, final_dev, tgrid_host, n_grid, use_cfg, t_round, a, (hipStream_t)stream, dense_elems(e, a), nullptr, method},
                          GuidancePlan::of_cache(&cc), nullptr);
}

// the single evaluations the host loop of transport/cache.py is built from
extern "C" int lt_forward_cached(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, int32_t mode, int32_t use_cfg, const lt_step_args* a,
                                 double* sums_host, void* stream) {
    LT_REQUIRE(e && x_dev && t_dev && a, "lt_forward_cached: null argument");
    LT_REQUIRE(mode >= LT_CACHE_PROBE && mode <= LT_CACHE_REUSE, "lt_forward_cached: mode %d is not LT_CACHE_PROBE, LT_CACHE_RUN or LT_CACHE_REUSE", mode);
    LT_REQUIRE(mode == LT_CACHE_PROBE ? sums_host != nullptr : out_dev != nullptr, "lt_forward_cached: null argument (%s)",
               mode == LT_CACHE_PROBE ? "sums_host" : "out_dev");
    hipStream_t s = (hipStream_t)stream;
    if (refuse_if_capturing(s, "lt_forward_cached")) return 2;
    LtOptScope opt_scope(&e->opts);
    if (check_cached_call(e, "lt_forward_cached", a, use_cfg)) return 2;
    int want[4];
    stored_sig_of(e, LT_STORED_RESIDUAL, a, use_cfg, want);
    if (mode == LT_CACHE_REUSE)
        LT_REQUIRE(same_sig(e->cache_res, want), "lt_forward_cached: LT_CACHE_REUSE without a stored residual of this shape (batch %d, latent %dx%d, cfg %d): an LT_CACHE_RUN "
                   "evaluation under the same conditioning comes first", a->batch, a->latent_h, a->latent_w, use_cfg ? 1 : 0);
    if (ensure_step_cache(e)) return 1;
    if (mode == LT_CACHE_PROBE) {
        if (int rc = cache_probe(e, x_dev, t_dev, a, use_cfg, s)) return rc;
        sums_host[0] = e->c_sums_host[0]; sums_host[1] = e->c_sums_host[1];
        return 0;
    }
    if (mode == LT_CACHE_REUSE) return forward_graphed(e, x_dev, t_dev, out_dev, a, use_cfg, s, {LT_KIND_CACHE_APPLY});
    return forward_rewriting(e, LT_STORED_RESIDUAL, x_dev, t_dev, out_dev, a, use_cfg, s, {LT_KIND_CACHE_BLOCKS});
}

// lt_sample_ode on a packed batch: z, every trajectory slot and the final state are flat buffers of the size list's layout (packed.hip)
extern "C" int lt_sample_ode_packed(lt_engine* e, const void* z_flat_dev, const int32_t* hw_host, void* traj_flat_dev, void* final_flat_dev,
                                    const float* tgrid_host, int32_t n_grid, int32_t method, int32_t use_cfg, int32_t t_round, const lt_step_args* a,
                                    void* stream) {
    return sample_plain(e, "lt_sample_ode_packed", {z_flat_dev, traj_flat_dev, final_flat_dev, tgrid_host, n_grid, use_cfg, t_round, a, (hipStream_t)stream, 0,
                        nullptr, method}, hw_host, true, nullptr);
}

// ---- inpainting: the fixed-grid loop with the blend in each step's closing combine --------------------------------------
extern "C" int lt_sample_ode_masked(lt_engine* e, const void* z_dev, const void* mask_dev, const void* x1_dev, const void* noise_dev, void* traj_dev,
                                    void* final_dev, const float* tgrid_host, int32_t n_grid, int32_t method, int32_t use_cfg, int32_t t_round,
                                    const lt_step_args* a, void* stream) {
    const MaskedBlend mb{mask_dev, x1_dev, noise_dev};
    return sample_plain(e, "lt_sample_ode_masked", {z_dev, traj_dev, final_dev, tgrid_host, n_grid, use_cfg, t_round, a, (hipStream_t)stream, 0, nullptr, method},
                        nullptr, false, &mb);
}

extern "C" int lt_sample_ode_masked_packed(lt_engine* e, const void* z_flat_dev, const int32_t* hw_host, const void* mask_flat_dev,
                                           const void* x1_flat_dev, const void* noise_flat_dev, void* traj_flat_dev, void* final_flat_dev,
                                           const float* tgrid_host, int32_t n_grid, int32_t method, int32_t use_cfg, int32_t t_round,
                                           const lt_step_args* a, void* stream) {
    const MaskedBlend mb{mask_flat_dev, x1_flat_dev, noise_flat_dev};
    return sample_plain(e, "lt_sample_ode_masked_packed", {z_flat_dev, traj_flat_dev, final_flat_dev, tgrid_host, n_grid, use_cfg, t_round, a,
                        (hipStream_t)stream, 0, nullptr, method}, hw_host, true, &mb);
}

// ---- guidance schedules: a scale per stage, conditional-only stages at half the rows --------------------------------------
namespace {

// what a guided evaluation on the two halves of a prepared conditioning needs, refused by name before anything is written
int check_guided_halves(const lt_engine* e, const char* who, const lt_step_args* a) {
    LT_REQUIRE(a->batch % 2 == 0, "%s: guidance needs an even batch (cond + uncond rows), got %d", who, a->batch);
    LT_REQUIRE(e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): its captions belong to "
               "one cond and one uncond row, there is no conditional half to evaluate alone", who);
    LT_REQUIRE(e->prompt_B == a->batch, "%s: %s was called for batch %d, step has batch %d", who,
               e->v.labels ? "lt_prepare_labels" : "lt_prepare_prompt", e->prompt_B, a->batch);
    return 0;
}

// the parameters of the rescale / norm-limit rule
int check_rule(const char* who, float rescale, float norm_limit) {
    LT_REQUIRE(std::isfinite(rescale) && rescale >= 0.f && rescale <= 1.f, "%s: rescale %g is not a blend in [0, 1]", who, (double)rescale);
    LT_REQUIRE(!std::isnan(norm_limit) && norm_limit > 0.f, "%s: norm_limit %g is not above 0 (+inf switches the limit off)", who, (double)norm_limit);
    return 0;
}

// the form and the parameters of projected guidance
int check_project(const char* who, int form, float eta, float momentum, float norm_threshold) {
    LT_REQUIRE(form == LT_PROJECT_APG || form == LT_PROJECT_ZERO_STAR, "%s: form %d is not LT_PROJECT_APG (1) or LT_PROJECT_ZERO_STAR (2)", who, form);
    if (form != LT_PROJECT_APG) return 0;  // (CFG-Zero* reads none of the three)
    LT_REQUIRE(std::isfinite(eta), "%s: eta %g is not finite", who, (double)eta);
    LT_REQUIRE(std::fabs(momentum) < 1.f, "%s: momentum %g is not inside (-1, 1)", who, (double)momentum);
    LT_REQUIRE(!std::isnan(norm_threshold) && norm_threshold > 0.f, "%s: norm_threshold %g is not above 0 (+inf switches the clip off)", who,
               (double)norm_threshold);
    return 0;
}

// what every call with a scale per evaluation checks behind the shape, before anything is written: the batch, the `intervals * stages` scales,
// the rule's parameters (`rule` = { rescale, norm limit } or null) and the prepared conditioning
int check_guided_table(const lt_engine* e, const char* who, const lt_step_args* a, const float* cfg_host, int intervals, int stages, const float* rule) {
    LT_REQUIRE(a->batch % 2 == 0, "%s: guidance needs an even batch (cond + uncond rows), got %d", who, a->batch);
    for (int i = 0; i < intervals * stages; ++i)
        LT_REQUIRE(std::isfinite(cfg_host[i]), "%s: the scale of stage %d of interval %d is not finite", who, i % stages, i / stages);
    if (rule && check_rule(who, rule[0], rule[1])) return 2;
    return check_guided_halves(e, who, a);
}

// the flag table of guidance reuse, one flag per scale: 0 / 1, and at the scales other than 1 a refresh before the first reuse
// (at scale 1 exactly the stage is conditional-only under either flag)
int check_reuse_flags(const char* who, const float* cfg_host, const int32_t* reuse_host, int ncalls) {
    bool stored = false;
    for (int i = 0; i < ncalls; ++i) {
        LT_REQUIRE(reuse_host[i] == 0 || reuse_host[i] == 1, "%s: reuse flag %d of evaluation %d is not 0 (refresh) or 1 (reuse)", who, reuse_host[i], i);
        if (cfg_host[i] == 1.0f) continue;
        if (reuse_host[i] == 0) stored = true;
        LT_REQUIRE(stored, "%s: evaluation %d reuses the cond - uncond difference, but no refresh evaluation (flag 0 at a scale other than 1) comes "
                   "before it in this call", who, i);
    }
    return 0;
}

// Every fixed-grid call with a scale per evaluation: the plan's form says which (lt_sample_ode_cfg_schedule, _rule, _reuse, _slg, _pag, _project)
int sample_cfg_table(lt_engine* e, const char* who, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int n_grid, int method,
                     const GuidancePlan& plan, int t_round, const lt_step_args* a, hipStream_t s) {
    LT_REQUIRE(e && z_dev && tgrid_host && plan.table && a, "%s: null argument", who);
    LT_REQUIRE(plan.form != LT_PLAN_REUSE || plan.reuse, "%s: null argument (reuse_host: one int32 flag per stage)", who);
    LT_REQUIRE(plan.form != LT_PLAN_SLG || plan.slg, "%s: null argument (slg_host: one skip-layer scale per stage)", who);
    if (refuse_if_capturing(s, who)) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    if (check_grid_method(who, n_grid, method, false, "")) return 2;
    if (check_step_shape(e, who, a)) return 2;
    const int stages = method == LT_ODE_EULER ? 1 : (method == LT_ODE_MIDPOINT ? 2 : 4);
    const int ncalls = (n_grid - 1) * stages;
    if (check_guided_table(e, who, a, plan.table, n_grid - 1, stages, plan.rule)) return 2;
    if (plan.form == LT_PLAN_REUSE && check_reuse_flags(who, plan.table, plan.reuse, ncalls)) return 2;
    if (plan.form == LT_PLAN_REUSE && ensure_delta(e)) return 1;
    if (plan.projected()) {
        if (check_project(who, plan.project_form, plan.par[0], plan.par[1], plan.par[2])) return 2;
        LT_REQUIRE(plan.zero_init >= 0 && plan.zero_init < n_grid - 1, "%s: zero_init %d leaves no interval of the %d to integrate "
                   "(0 .. n_grid - 2)", who, plan.zero_init, n_grid - 1);
        LT_REQUIRE(plan.form == LT_PLAN_PROJECT_ZERO_STAR || plan.zero_init == 0, "%s: zero_init %d belongs to CFG-Zero* (form %d), not to "
                   "APG", who, plan.zero_init, LT_PROJECT_ZERO_STAR);
        if (ensure_project(e)) return 1;
    }
    if (plan.form == LT_PLAN_SLG) {
        for (int i = 0; i < ncalls; ++i)
            LT_REQUIRE(std::isfinite(plan.slg[i]), "%s: the skip-layer scale of stage %d of interval %d is not finite", who, i % stages, i / stages);
        if (check_layer_sets(e, who, plan.skip, plan.n_skip, plan.perturb, plan.n_perturb)) return 2;
        if (check_blur_sets(e, who, plan.skip, plan.n_skip, plan.blur, plan.n_blur, plan.blur_sigma)) return 2;
        if (check_blur_radius(e, who, a, plan.n_blur, plan.blur_sigma)) return 2;  // (before the first stage, whatever its scale)
        LT_REQUIRE(plan.n_blur == 0 || e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): blurred queries do not serve it", who);
        if (plan.pag && plan.n_skip == 0 && plan.n_perturb == 0 && plan.n_blur == 0)
            for (int i = 0; i < ncalls; ++i)
                LT_REQUIRE(plan.slg[i] == 0.0f, "%s: both layer sets are empty, and stage %d of interval %d has a non-zero scale: the third "
                           "prediction would be the conditional one", who, i % stages, i / stages);
        if (ensure_skip_buf(e)) return 1;
        if (plan.n_blur > 0 && ensure_blur(e, plan.blur_sigma, s)) return 1;
    }
    ProjectScope form_scope(e, plan.project_form);
    return ode_fixed_grid(e, {z_dev, traj_dev, final_dev, tgrid_host, n_grid, 1, t_round, a, s, dense_elems(e, a), nullptr, method}, plan, nullptr);
}

}  // namespace

extern "C" int lt_sample_ode_cfg_schedule(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                          int32_t method, const float* cfg_host, int32_t t_round, const lt_step_args* a, void* stream) {
    return sample_cfg_table(e, "lt_sample_ode_cfg_schedule", z_dev, traj_dev, final_dev, tgrid_host, n_grid, method, GuidancePlan::of_table(cfg_host),
                            t_round, a, (hipStream_t)stream);
}

// ---- rescaled and norm-limited guidance: a per-sample factor on every guided stage -------------------------------------------
extern "C" int lt_sample_ode_cfg_rule(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                      int32_t method, const float* cfg_host, float rescale, float norm_limit, int32_t t_round, const lt_step_args* a,
                                      void* stream) {
    const float rule[2] = {rescale, norm_limit};
    return sample_cfg_table(e, "lt_sample_ode_cfg_rule", z_dev, traj_dev, final_dev, tgrid_host, n_grid, method, GuidancePlan::of_rule(cfg_host, rule),
                            t_round, a, (hipStream_t)stream);
}

// One guided evaluation under the rule, at a->cfg_scale.  The three parameters reach the engine's fixed device words through a launch in
// front of the evaluation.  Refused on a capturing stream: a recorded evaluation of this kind has no test behind it yet.
extern "C" int lt_forward_cfg_rule(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, float rescale, float norm_limit,
                                   const lt_step_args* a, void* stream) {
    const char* who = "lt_forward_cfg_rule";
    LT_REQUIRE(e && x_dev && t_dev && out_dev && a, "%s: null argument", who);
    if (refuse_if_capturing((hipStream_t)stream, who)) return 2;
    LtOptScope opt_scope(&e->opts);
    if (check_step_shape(e, who, a)) return 2;
    LT_REQUIRE(std::isfinite(a->cfg_scale), "%s: the scale is not finite", who);
    if (check_rule(who, rescale, norm_limit)) return 2;
    if (check_guided_halves(e, who, a)) return 2;
    if (launch_guidance_params_store(e->g_cfg, a->cfg_scale, rescale, norm_limit, (hipStream_t)stream)) return 1;
    return forward_graphed(e, x_dev, t_dev, out_dev, a, 1, (hipStream_t)stream, {LT_KIND_RULE, nullptr, e->g_cfg});
}

// ---- projected guidance: APG and CFG-Zero*, the forms that need inner products of the two predictions ------------------------
extern "C" int lt_sample_ode_cfg_project(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                         int32_t method, const float* cfg_host, int32_t form, float eta, float momentum, float norm_threshold,
                                         int32_t zero_init, int32_t t_round, const lt_step_args* a, void* stream) {
    const GuidancePlan plan = GuidancePlan::of_project(cfg_host, form == LT_PROJECT_APG, form, eta, momentum, norm_threshold, zero_init);
    return sample_cfg_table(e, "lt_sample_ode_cfg_project", z_dev, traj_dev, final_dev, tgrid_host, n_grid, method, plan, t_round, a, (hipStream_t)stream);
}

// One guided evaluation under a projected form, at a->cfg_scale.  The four parameters reach the engine's fixed device words through a launch
// in front of the evaluation (the scale from there into e->g_cfg[0], as every device scale travels).  keep_momentum: 0 zeroes APG's momentum
// first, 1 continues from the stored one - which must be of this call's shape.
extern "C" int lt_forward_cfg_project(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, int32_t form, float eta, float momentum,
                                      float norm_threshold, int32_t keep_momentum, const lt_step_args* a, void* stream) {
    const char* who = "lt_forward_cfg_project";
    hipStream_t s = (hipStream_t)stream;
    LT_REQUIRE(e && x_dev && t_dev && out_dev && a, "%s: null argument", who);
    if (refuse_if_capturing(s, who)) return 2;  // (the first call allocates the buffers)
    LtOptScope opt_scope(&e->opts);
    if (check_step_shape(e, who, a)) return 2;
    LT_REQUIRE(std::isfinite(a->cfg_scale), "%s: the scale is not finite", who);
    if (check_project(who, form, eta, momentum, norm_threshold)) return 2;
    LT_REQUIRE(keep_momentum == 0 || keep_momentum == 1, "%s: keep_momentum %d is not 0 (start from zero) or 1 (continue)", who, keep_momentum);
    LT_REQUIRE(form == LT_PROJECT_APG || keep_momentum == 0, "%s: keep_momentum belongs to APG; CFG-Zero* carries no momentum", who);
    if (check_guided_halves(e, who, a)) return 2;
    if (keep_momentum && check_stored(e, who, LT_STORED_MOMENTUM, a, "momentum", "continue from", "no projected APG evaluation was made")) return 2;
    if (ensure_project(e)) return 1;
    if (form != LT_PROJECT_APG) { eta = 1.f; momentum = 0.f; norm_threshold = INFINITY; }  // (not read; the words hold no leftovers)
    if (launch_guidance_project_params_store(e->p_par, a->cfg_scale, eta, momentum, norm_threshold, s)) return 1;
    if (form == LT_PROJECT_APG && !keep_momentum && zero_momentum(e, a, s)) return 1;
    ProjectScope form_scope(e, form);
    return forward_rewriting(e, form == LT_PROJECT_APG ? LT_STORED_MOMENTUM : LT_STORED_NONE, x_dev, t_dev, out_dev, a, 1, s, {LT_KIND_RULE, nullptr, e->p_par});
}

// ---- guidance reuse: the cond - uncond difference taken on refresh stages, reused on half-row stages in between ----------------
extern "C" int lt_sample_ode_cfg_reuse(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                       int32_t method, const float* cfg_host, const int32_t* reuse_host, int32_t t_round, const lt_step_args* a,
                                       void* stream) {
    return sample_cfg_table(e, "lt_sample_ode_cfg_reuse", z_dev, traj_dev, final_dev, tgrid_host, n_grid, method,
                            GuidancePlan::of_reuse(cfg_host, reuse_host), t_round, a, (hipStream_t)stream);
}

// One guided evaluation at a->cfg_scale that stores the difference (mode 0: lt_forward_cfg's result) or evaluates the cond rows and reuses it
// (mode 1).  The scale reaches the engine's fixed device word through a launch in front of the evaluation, as in lt_forward_cfg_rule.
extern "C" int lt_forward_cfg_reuse(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, int32_t mode, const lt_step_args* a,
                                    void* stream) {
    const char* who = "lt_forward_cfg_reuse";
    LT_REQUIRE(e && x_dev && t_dev && out_dev && a, "%s: null argument", who);
    if (refuse_if_capturing((hipStream_t)stream, who)) return 2;  // (the first call allocates the difference buffer)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(mode == 0 || mode == 1, "%s: mode %d is not 0 (guide and store the difference) or 1 (reuse it)", who, mode);
    if (check_step_shape(e, who, a)) return 2;
    LT_REQUIRE(std::isfinite(a->cfg_scale), "%s: the scale is not finite", who);
    if (check_guided_halves(e, who, a)) return 2;
    if (mode == 1 && check_stored(e, who, LT_STORED_DELTA, a, "cond - uncond difference", "reuse", "none was taken (mode 0)")) return 2;
    if (ensure_delta(e)) return 1;
    if (launch_guidance_params_store(e->g_cfg, a->cfg_scale, 0.f, INFINITY, (hipStream_t)stream)) return 1;
    return forward_rewriting(e, mode ? LT_STORED_NONE : LT_STORED_DELTA, x_dev, t_dev, out_dev, a, 1, (hipStream_t)stream,
                             {mode ? LT_KIND_REUSE_AGAIN : LT_KIND_REUSE_STORE, nullptr, e->g_cfg});
}

// ---- skip-layer guidance: a third prediction with a set of blocks left out, pushed away from -----------------------------------
extern "C" int lt_sample_ode_cfg_slg(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                     int32_t method, const float* cfg_host, const float* slg_host, const int32_t* skip_host, int32_t n_skip,
                                     int32_t t_round, const lt_step_args* a, void* stream) {
    return sample_cfg_table(e, "lt_sample_ode_cfg_slg", z_dev, traj_dev, final_dev, tgrid_host, n_grid, method,
                            GuidancePlan::of_slg(cfg_host, slg_host, skip_host, n_skip, nullptr, 0, false), t_round, a, (hipStream_t)stream);
}

// ---- perturbed-attention guidance: the third prediction runs the blocks of P with the identity as their attention map -----------
extern "C" int lt_sample_ode_cfg_pag(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                     int32_t method, const float* cfg_host, const float* pag_host, const int32_t* skip_host, int32_t n_skip,
                                     const int32_t* perturb_host, int32_t n_perturb, int32_t t_round, const lt_step_args* a, void* stream) {
    return sample_cfg_table(e, "lt_sample_ode_cfg_pag", z_dev, traj_dev, final_dev, tgrid_host, n_grid, method,
                            GuidancePlan::of_slg(cfg_host, pag_host, skip_host, n_skip, perturb_host, n_perturb, true), t_round, a, (hipStream_t)stream);
}

// ---- smoothed-energy guidance: the third prediction runs the blocks of Q on Gaussian-blurred queries ----------------------------
extern "C" int lt_sample_ode_cfg_seg(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                     int32_t method, const float* cfg_host, const float* seg_host, const int32_t* skip_host, int32_t n_skip,
                                     const int32_t* blur_host, int32_t n_blur, float sigma, int32_t t_round, const lt_step_args* a, void* stream) {
    return sample_cfg_table(e, "lt_sample_ode_cfg_seg", z_dev, traj_dev, final_dev, tgrid_host, n_grid, method,
                            GuidancePlan::of_seg(cfg_host, seg_host, skip_host, n_skip, blur_host, n_blur, sigma), t_round, a, (hipStream_t)stream);
}

// One guided evaluation at (cfg_scale, slg_scale): the degraded evaluation of the cond rows - the blocks of S left out, the blocks of P
// perturbed - then all rows (the cond rows alone at cfg_scale 1 exactly).  slg_scale 0: lt_forward_cfg at cfg_scale.  The scales reach the
// engine's fixed device words through a launch in front.  pag: lt_forward_cfg_pag (both sets, either may be empty, not both at a scale != 0)
// seg: lt_forward_cfg_seg - the blur set at width sigma in place of the perturb set
static int forward_cfg_sets(lt_engine* e, const char* who, bool pag, const void* x_dev, const float* t_dev, void* out_dev, float cfg_scale,
                            float slg_scale, const int32_t* skip_host, int32_t n_skip, const int32_t* perturb_host, int32_t n_perturb,
                            const lt_step_args* a, void* stream, const int32_t* blur_host = nullptr, int32_t n_blur = 0, float sigma = 0.f,
                            bool seg = false) {
    hipStream_t s = (hipStream_t)stream;
    LT_REQUIRE(e && x_dev && t_dev && out_dev && a, "%s: null argument", who);
    if (refuse_if_capturing(s, who)) return 2;  // (the first call allocates the skip buffer)
    LtOptScope opt_scope(&e->opts);
    if (check_step_shape(e, who, a)) return 2;
    LT_REQUIRE(std::isfinite(cfg_scale), "%s: the scale is not finite", who);
    LT_REQUIRE(std::isfinite(slg_scale), "%s: the %s scale is not finite", who, seg ? "smoothed-energy" : pag ? "perturbed-attention" : "skip-layer");
    if (check_guided_halves(e, who, a)) return 2;
    if (check_layer_sets(e, who, skip_host, n_skip, perturb_host, n_perturb)) return 2;
    if (seg && check_blur_sets(e, who, skip_host, n_skip, blur_host, n_blur, sigma)) return 2;
    if (seg && check_blur_radius(e, who, a, n_blur, sigma)) return 2;
    LT_REQUIRE(n_blur == 0 || e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): blurred queries do not serve it", who);
    LT_REQUIRE(!pag || n_skip > 0 || n_perturb > 0 || n_blur > 0 || slg_scale == 0.f, "%s: both layer sets are empty at a non-zero scale: the third prediction "
               "would be the conditional one", who);
    lt_step_args own = *a;
    own.cfg_scale = cfg_scale;
    if (slg_scale == 0.f) return forward_graphed(e, x_dev, t_dev, out_dev, &own, 1, s);  // lt_forward_cfg's launches and result
    if (ensure_skip_buf(e)) return 1;
    if (n_blur > 0 && ensure_blur(e, sigma, s)) return 1;
    if (launch_slg_params_store(e->g_cfg, cfg_scale, slg_scale, s)) return 1;
    const GuidancePlan sets = seg ? GuidancePlan::of_seg(nullptr, nullptr, skip_host, n_skip, blur_host, n_blur, sigma)
                                  : GuidancePlan::of_slg(nullptr, nullptr, skip_host, n_skip, perturb_host, n_perturb, pag);
    return forward_slg_pair(e, who, sets, x_dev, t_dev, out_dev, &own, s, cfg_scale == 1.0f ? LT_KIND_SLG_COND : LT_KIND_SLG_GUIDED, e->g_cfg, nullptr);
}

extern "C" int lt_forward_cfg_seg(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, float cfg_scale, float seg_scale,
                                  const int32_t* skip_host, int32_t n_skip, const int32_t* blur_host, int32_t n_blur, float sigma, const lt_step_args* a,
                                  void* stream) {
    return forward_cfg_sets(e, "lt_forward_cfg_seg", true, x_dev, t_dev, out_dev, cfg_scale, seg_scale, skip_host, n_skip, nullptr, 0, a, stream,
                            blur_host, n_blur, sigma, true);
}

extern "C" int lt_forward_cfg_slg(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, float cfg_scale, float slg_scale,
                                  const int32_t* skip_host, int32_t n_skip, const lt_step_args* a, void* stream) {
    return forward_cfg_sets(e, "lt_forward_cfg_slg", false, x_dev, t_dev, out_dev, cfg_scale, slg_scale, skip_host, n_skip, nullptr, 0, a, stream);
}

extern "C" int lt_forward_cfg_pag(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, float cfg_scale, float pag_scale,
                                  const int32_t* skip_host, int32_t n_skip, const int32_t* perturb_host, int32_t n_perturb, const lt_step_args* a,
                                  void* stream) {
    return forward_cfg_sets(e, "lt_forward_cfg_pag", true, x_dev, t_dev, out_dev, cfg_scale, pag_scale, skip_host, n_skip, perturb_host, n_perturb, a,
                            stream);
}

// ---- linear multistep sampling: one evaluation per interval, the earlier slopes reused (multistep.hip) -------------------------
namespace {

// what both multistep calls check of the grid and the weight table, before anything is written
int check_multistep(const char* who, int n_grid, const float* coef_host, int corrector) {
    LT_REQUIRE(n_grid >= 2, "%s: need at least 2 grid points", who);
    LT_REQUIRE(corrector == 0 || corrector == 1, "%s: corrector %d is not 0 (Adams-Bashforth) or 1 (with the Adams-Moulton corrector)", who, corrector);
    for (int i = 0; i + 1 < n_grid; ++i) {
        const float* row = coef_host + (size_t)i * 8;
        for (int j = 0; j < 8; ++j)
            LT_REQUIRE(std::isfinite(row[j]), "%s: weight %c[%d] of interval %d is not finite", who, j < 4 ? 'a' : 'b', j % 4, i);
        const int need = std::max(corrector ? multistep_used(row) : 0, multistep_used(row + 4));
        LT_REQUIRE(need <= std::min(i + 1, 4), "%s: interval %d names %d slopes, %d evaluations have been made by then", who, i, need, i + 1);
    }
    return 0;
}

// The multistep loop on a state of n elements (elementwise, so a packed batch's flat state runs through it as it is).  Evaluation i runs at
// tgrid[i] on the predicted state and overwrites ring slot i % 4 of e->kbuf, the slot of f_{i-4}.  Without a corrector the state ping-pongs
// through e->ys like a fixed-grid step; with one, ys holds the corrected states y_i and e->ymid the predictor p_{i+1} the next evaluation
// reads.  The plan's tail is committed behind the stage times and applied exactly as ode_fixed_grid does (stages = 1).
int ode_multistep(lt_engine* e, const GridCall& c, const GuidancePlan& plan) {
    const lt_step_args* a = c.a;
    hipStream_t s = c.s;
    const float *tgrid_host = c.tgrid, *coef_host = c.coef;
    const int B = a->batch, ncalls = c.n_grid - 1, corrector = c.corrector;
    const long long n = c.n;
    const bool bf = a->io_dtype == LT_BF16;
    const int nsent = ncalls * B + plan.tail_floats(ncalls);
    float* tp = e->times.begin(nsent, s);
    if (!tp) return 1;
    for (int i = 0; i < ncalls; ++i) {
        const float tv = (c.t_round && bf) ? bf16_round_host(tgrid_host[i]) : tgrid_host[i];
        for (int b = 0; b < B; ++b) tp[(size_t)i * B + b] = tv;
    }
    plan.fill_tail(tp + GuidancePlan::table_offset(ncalls, B), ncalls);
    if (e->times.commit(nsent, s) || apply_plan(e, plan, a, ncalls, s)) return 1;
    Trajectory tr{e, a, c.use_cfg, s, (size_t)n * (bf ? 2 : 4), c.pc, plan, ncalls};
    if (tr.start(c.z, c.traj, true)) return 1;
    const int dt_code = bf ? 1 : 0;
    const void* p = tr.y0();  // p_i, the state evaluation i reads: p_0 = z
    for (int i = 0; i < ncalls; ++i) {
        const float* row = coef_host + (size_t)i * 8;
        if (tr.eval(p, i, e->kbuf[i % 4])) return 1;
        const int nslopes = std::max(1, std::max(corrector ? multistep_used(row) : 0, multistep_used(row + 4)));  // (<= min(i + 1, 4): check_multistep)
        const void* k[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int j = 0; j < nslopes; ++j) k[j] = e->kbuf[(i - j) % 4];  // newest first
        if (!corrector) {  // y_i = p_i; p_{i+1} is the next recorded state
            if (launch_ode_multistep(tr.y0(), k, nslopes, nullptr, row + 4, 0, nullptr, tr.y1(), n, dt_code, s)) return 1;
            if (tr.advance(i + 1)) return 1;
            p = tr.y0();
        } else if (multistep_used(row) == 0) {  // a row without corrector weights: y_i = p_i
            if (i > 0) {  // p_i lies in ymid, ys[cur] holds y_{i-1}: p_i becomes the stored y_i, recorded in slot i (at step 0 ys[0] = z is both)
                LT_CHECK_HIP(hipMemcpyAsync(tr.y1(), e->ymid, tr.sbytes, hipMemcpyDeviceToDevice, s));
                if (tr.advance(i)) return 1;
            }
            if (launch_ode_multistep(tr.y0(), k, nslopes, nullptr, row + 4, 0, nullptr, e->ymid, n, dt_code, s)) return 1;
            p = e->ymid;
        } else {  // y_i from y_{i-1}, recorded in slot i; p_{i+1} from the stored y_i
            if (launch_ode_multistep(tr.y0(), k, nslopes, row, row + 4, 1, tr.y1(), e->ymid, n, dt_code, s)) return 1;
            if (tr.advance(i)) return 1;
            p = e->ymid;
        }
    }
    if (!corrector) return tr.finish(c.final);
    // the result p_N lies in ymid: the last slot of the record, and the final state
    if (c.traj) LT_CHECK_HIP(hipMemcpyAsync((char*)c.traj + (size_t)ncalls * tr.sbytes, e->ymid, tr.sbytes, hipMemcpyDeviceToDevice, s));
    if (c.final) LT_CHECK_HIP(hipMemcpyAsync(c.final, e->ymid, tr.sbytes, hipMemcpyDeviceToDevice, s));
    return tr.finish(nullptr);
}

}  // namespace

extern "C" int lt_sample_ode_multistep(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                       const float* coef_host, int32_t corrector, const float* cfg_host, float rescale, float norm_limit,
                                       int32_t use_cfg, int32_t t_round, const lt_step_args* a, void* stream) {
    const char* who = "lt_sample_ode_multistep";
    LT_REQUIRE(e && z_dev && tgrid_host && coef_host && a, "%s: null argument", who);
    if (check_multistep(who, n_grid, coef_host, corrector)) return 2;  // (the table and the flags first: host arguments, no engine state read)
    const bool rule_on = !(rescale == 0.f && norm_limit == INFINITY);
    LT_REQUIRE(use_cfg || !cfg_host, "%s: a guidance table with use_cfg = 0 (the table scales forward_with_cfg)", who);
    LT_REQUIRE(use_cfg || !rule_on, "%s: a rescale / norm-limit rule with use_cfg = 0 (the rule acts on guided evaluations)", who);
    if (refuse_if_capturing((hipStream_t)stream, who)) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    if (check_step_shape(e, who, a)) return 2;
    GridCall c{z_dev, traj_dev, final_dev, tgrid_host, n_grid, use_cfg, t_round, a, (hipStream_t)stream, dense_elems(e, a), nullptr, 0, coef_host, corrector};
    if (!cfg_host && !rule_on) return ode_multistep(e, c, {});
    // a scale per evaluation [and the rule]: the checks of sample_cfg_table
    std::vector<float> constant;
    if (!cfg_host) {  // the rule at one scale
        constant.assign(n_grid - 1, a->cfg_scale);
        cfg_host = constant.data();
    }
    const float rule[2] = {rescale, norm_limit};
    if (check_guided_table(e, who, a, cfg_host, n_grid - 1, 1, rule_on ? rule : nullptr)) return 2;
    c.use_cfg = 1;
    return ode_multistep(e, c, rule_on ? GuidancePlan::of_rule(cfg_host, rule) : GuidancePlan::of_table(cfg_host));
}

// lt_sample_ode_multistep with a scale and a reuse flag per evaluation: the same body, the checks of lt_sample_ode_cfg_reuse
extern "C" int lt_sample_ode_multistep_cfg_reuse(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host,
                                                 int32_t n_grid, const float* coef_host, int32_t corrector, const float* cfg_host,
                                                 const int32_t* reuse_host, int32_t t_round, const lt_step_args* a, void* stream) {
    const char* who = "lt_sample_ode_multistep_cfg_reuse";
    LT_REQUIRE(e && z_dev && tgrid_host && coef_host && cfg_host && a, "%s: null argument", who);
    LT_REQUIRE(reuse_host, "%s: null argument (reuse_host: one int32 flag per evaluation)", who);
    if (check_multistep(who, n_grid, coef_host, corrector)) return 2;
    if (refuse_if_capturing((hipStream_t)stream, who)) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    if (check_step_shape(e, who, a)) return 2;
    if (check_guided_table(e, who, a, cfg_host, n_grid - 1, 1, nullptr)) return 2;
    if (check_reuse_flags(who, cfg_host, reuse_host, n_grid - 1)) return 2;
    if (ensure_delta(e)) return 1;
    return ode_multistep(e, {z_dev, traj_dev, final_dev, tgrid_host, n_grid, 1, t_round, a, (hipStream_t)stream, dense_elems(e, a), nullptr, 0, coef_host, corrector},
                         GuidancePlan::of_reuse(cfg_host, reuse_host));
}

// lt_sample_ode_multistep on a packed batch: z, every trajectory slot and the final state are flat buffers of the size list's layout (packed.hip)
extern "C" int lt_sample_ode_multistep_packed(lt_engine* e, const void* z_flat_dev, const int32_t* hw_host, void* traj_flat_dev, void* final_flat_dev,
                                              const float* tgrid_host, int32_t n_grid, const float* coef_host, int32_t corrector, int32_t use_cfg,
                                              int32_t t_round, const lt_step_args* a, void* stream) {
    const char* who = "lt_sample_ode_multistep_packed";
    LT_REQUIRE(e && z_flat_dev && hw_host && tgrid_host && coef_host && a, "%s: null argument", who);
    if (check_multistep(who, n_grid, coef_host, corrector)) return 2;
    if (refuse_if_capturing((hipStream_t)stream, who)) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    PackedCall pc{};
    if (int rc = packed_call_begin(e, who, hw_host, a, use_cfg, &pc, (hipStream_t)stream)) return rc;
    return ode_multistep(e, {z_flat_dev, traj_flat_dev, final_flat_dev, tgrid_host, n_grid, use_cfg, t_round, a, (hipStream_t)stream, pc.elems, &pc, 0, coef_host,
                          corrector}, {});
}

// ---- multi-view (visual-anagram) sampling ------------------------------------------------------------------------------------------
void drop_views(lt_engine* e) {
    if (e->vw_perm) (void)hipFree(e->vw_perm);
    if (e->vw_iperm) (void)hipFree(e->vw_iperm);
    if (e->vw_hits) (void)hipFree(e->vw_hits);
    if (e->vw_vsign) (void)hipFree(e->vw_vsign);
    if (e->vw_isign) (void)hipFree(e->vw_isign);
    e->vw_perm = e->vw_iperm = e->vw_hits = nullptr;
    e->vw_vsign = e->vw_isign = nullptr;
    e->vw_V = e->vw_h = e->vw_w = 0;
}

extern "C" int lt_set_views(lt_engine* e, const int32_t* perm_dev, const float* vsign_host, const float* isign_host, int32_t V, int32_t latent_h,
                            int32_t latent_w, void* stream) {
    LT_REQUIRE(e, "lt_set_views: null engine");
    if (refuse_if_capturing((hipStream_t)stream, "lt_set_views")) return 2;  // (allocates, uploads host tables, synchronises)
    hipStream_t s = (hipStream_t)stream;
    const lt_config& c = e->cfg;
    LT_REQUIRE(c.variant == LT_VARIANT_NEXT_T2I, "lt_set_views: multi-view sampling drives the text-conditional Next-DiT (LT_VARIANT_NEXT_T2I) only; "
               "this engine is variant %d", c.variant);
    if (V == 0 && !perm_dev) {  // drop the tables (kernels of an earlier trajectory may still read them)
        LT_CHECK_HIP(hipStreamSynchronize(s));
        drop_views(e);
        return 0;
    }
    LT_REQUIRE(perm_dev && vsign_host && isign_host, "lt_set_views: null argument");
    LT_REQUIRE(V >= 1, "lt_set_views: V = %d views (need at least 1)", V);
    LT_REQUIRE(2 * (long long)V <= c.max_batch, "lt_set_views: %d views need a batch of 2 V = %d rows (view prompts + negative prompts), max_batch is %d", V,
               2 * V, c.max_batch);
    if (check_latent(e, "lt_set_views", latent_h, latent_w)) return 2;
    const int C = c.in_channels, HW = latent_h * latent_w;
    LT_REQUIRE(HW % 4 == 0, "lt_set_views: H * W = %d must be a multiple of 4", HW);
    for (int i = 0; i < V * C; ++i)
        LT_REQUIRE((vsign_host[i] == 1.f || vsign_host[i] == -1.f) && (isign_host[i] == 1.f || isign_host[i] == -1.f),
                   "lt_set_views: sign of view %d, channel %d is not +1 / -1", i / C, i % C);
    LT_CHECK_HIP(hipStreamSynchronize(s));  // table upload may synchronise; kernels of an earlier trajectory may still read the old tables
    drop_views(e);
    const size_t tb = (size_t)V * HW * sizeof(int);
    auto fail = [&]() { drop_views(e); return 1; };
    if (hipMalloc((void**)&e->vw_perm, tb) != hipSuccess || hipMalloc((void**)&e->vw_iperm, tb) != hipSuccess ||
        hipMalloc((void**)&e->vw_hits, tb + sizeof(int)) != hipSuccess || hipMalloc((void**)&e->vw_vsign, (size_t)V * C * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&e->vw_isign, (size_t)V * C * sizeof(float)) != hipSuccess) {
        lt_set_error("lt_set_views: out of device memory for the tables of %d views of %d pixels", V, HW);
        return fail();
    }
    int bad = -1;
    if (hipMemcpyAsync(e->vw_perm, perm_dev, tb, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemsetAsync(e->vw_iperm, 0, tb, s) != hipSuccess ||
        hipMemcpyAsync(e->vw_vsign, vsign_host, (size_t)V * C * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(e->vw_isign, isign_host, (size_t)V * C * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_views_invert(e->vw_perm, e->vw_iperm, e->vw_hits, V, HW, s) ||
        hipMemcpyAsync(&bad, e->vw_hits + (size_t)V * HW, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        lt_set_error("lt_set_views: uploading the view tables failed");
        return fail();
    }
    if (bad != 0) {
        lt_set_error("lt_set_views: a view table is not a bijection on [0, %d): %d entries are out of range or name a pixel a second time", HW, bad);
        return fail();
    }
    e->vw_V = V; e->vw_h = latent_h; e->vw_w = latent_w;
    return 0;
}

extern "C" int lt_sample_views(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                               int32_t method, const lt_step_args* a, void* stream) {
    LT_REQUIRE(e && z_dev && tgrid_host && a, "lt_sample_views: null argument");
    if (refuse_if_capturing((hipStream_t)stream, "lt_sample_views")) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(e->cfg.variant == LT_VARIANT_NEXT_T2I, "lt_sample_views: multi-view sampling drives the text-conditional Next-DiT (LT_VARIANT_NEXT_T2I) "
               "only; this engine is variant %d", e->cfg.variant);
    LT_REQUIRE(n_grid >= 2, "lt_sample_views: need at least 2 grid points");
    LT_REQUIRE(method != LT_ODE_RK4, "lt_sample_views: rk4 is not a multi-view method (the reference steps views with its midpoint_solver; euler is the "
               "one-stage form)");
    LT_REQUIRE(method == LT_ODE_EULER || method == LT_ODE_MIDPOINT, "lt_sample_views: unknown method %d", method);
    LT_REQUIRE(e->vw_V >= 1, "lt_sample_views: no view tables (call lt_set_views first)");
    const int V = e->vw_V, B = 2 * V, C = e->cfg.in_channels, HW = e->vw_h * e->vw_w;
    LT_REQUIRE(a->batch == B, "lt_sample_views: %d views need a->batch = 2 V = %d (view prompts + negative prompts), got %d", V, B, a->batch);
    LT_REQUIRE(a->latent_h == e->vw_h && a->latent_w == e->vw_w, "lt_sample_views: the view tables are for a %dx%d latent, the call has %dx%d", e->vw_h,
               e->vw_w, a->latent_h, a->latent_w);
    // (not check_step_shape: batch and latent are checked against the view tables first, in this order - the tests pin the first error)
    LT_REQUIRE(a->io_dtype == LT_BF16 || a->io_dtype == LT_F32, "io_dtype must be bf16 or f32");
    LT_REQUIRE(B <= e->cfg.max_batch, "lt_sample_views: batch %d exceeds max_batch %d", B, e->cfg.max_batch);
    LT_REQUIRE(e->reg_Y == 0 && e->prompt_B == B, "lt_prepare_prompt was called for batch %d, step has batch %d (multi-view sampling needs the V view "
               "prompts followed by V rows of the negative prompt)", e->prompt_B, B);
    hipStream_t s = (hipStream_t)stream;
    const int stages = method == LT_ODE_EULER ? 1 : 2;
    const int ncalls = (n_grid - 1) * stages;
    const bool bf = a->io_dtype == LT_BF16;
    float* tp = e->times.begin(ncalls * B, s);
    if (!tp) return 1;
    // generate.py:212-219: t0, t1 are Python floats (the fp32 grid's values as doubles); dt = t1 - t0 and half_dt = 0.5 dt are doubles that
    // multiply a tensor as fp32 scalars; the stage times are torch.full((2,), t0) and torch.full((2,), t0 + half_dt): fp32 of the double
    std::vector<float> dts(n_grid - 1), hdts(n_grid - 1);
    for (int i = 0; i + 1 < n_grid; ++i) {
        const double t0 = tgrid_host[i], dt = (double)tgrid_host[i + 1] - t0, half_dt = 0.5 * dt;
        dts[i] = (float)dt;
        hdts[i] = (float)half_dt;
        const float ts[2] = {(float)t0, (float)(t0 + half_dt)};
        for (int k = 0; k < stages; ++k)
            for (int b = 0; b < B; ++b) tp[((size_t)i * stages + k) * B + b] = ts[k];
    }
    if (e->times.commit(ncalls * B, s)) return 1;
    // the state is ONE latent; one evaluation is ALL views: forward_with_cfg on 2 V rows, rows 0..V-1 = the viewed latents in ymid (it
    // reads the first half only)
    Trajectory tr{e, a, 1, s, (size_t)C * HW * (bf ? 2 : 4)};
    if (tr.start(z_dev, traj_dev, true)) return 1;
    const int dt_code = bf ? 1 : 0;
    for (int i = 0; i + 1 < n_grid; ++i) {
        void *y0 = tr.y0(), *y1 = tr.y1();
        const int c0 = i * stages;
        const void* slope = e->kbuf[0];
        if (launch_views_gather(y0, e->vw_perm, e->vw_vsign, nullptr, e->ymid, 0.f, V, C, HW, dt_code, s)) return 1;
        if (tr.eval(e->ymid, c0, e->kbuf[0])) return 1;
        if (method == LT_ODE_MIDPOINT) {
            if (launch_views_gather(y0, e->vw_perm, e->vw_vsign, e->kbuf[0], e->ymid, hdts[i], V, C, HW, dt_code, s)) return 1;
            if (tr.eval(e->ymid, c0 + 1, e->kbuf[1])) return 1;
            slope = e->kbuf[1];
        }
        if (launch_views_reduce(y0, slope, e->vw_iperm, e->vw_isign, y1, dts[i], V, C, HW, dt_code, s)) return 1;
        if (tr.advance(i + 1)) return 1;
    }
    return tr.finish(final_dev);
}

// Phase Upscale of the reference (generate.py:465-494): lt_sample_views' loop with midpoint_solver_extra (:222-262) as the stepping rule - the
// model input of each stage is the guided blend of views.hip, the interval's closing update is the same views_reduce
extern "C" int lt_sample_views_guided(lt_engine* e, const void* z_dev, const void* guidance_dev, const void* noise_dev, void* traj_dev, void* final_dev,
                                      const float* tgrid_host, const float* coef_host, int32_t n_grid, const lt_step_args* a, void* stream) {
    LT_REQUIRE(e && z_dev && guidance_dev && noise_dev && tgrid_host && coef_host && a, "lt_sample_views_guided: null argument");
    if (refuse_if_capturing((hipStream_t)stream, "lt_sample_views_guided")) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(e->cfg.variant == LT_VARIANT_NEXT_T2I, "lt_sample_views_guided: multi-view sampling drives the text-conditional Next-DiT "
               "(LT_VARIANT_NEXT_T2I) only; this engine is variant %d", e->cfg.variant);
    LT_REQUIRE(n_grid >= 2, "lt_sample_views_guided: need at least 2 grid points");
    LT_REQUIRE(e->vw_V >= 1, "lt_sample_views_guided: no view tables (call lt_set_views first)");
    const int V = e->vw_V, B = 2 * V, C = e->cfg.in_channels, HW = e->vw_h * e->vw_w;
    LT_REQUIRE(a->batch == B, "lt_sample_views_guided: %d views need a->batch = 2 V = %d (view prompts + negative prompts), got %d", V, B, a->batch);
    LT_REQUIRE(a->latent_h == e->vw_h && a->latent_w == e->vw_w, "lt_sample_views_guided: the view tables are for a %dx%d latent, the call has %dx%d",
               e->vw_h, e->vw_w, a->latent_h, a->latent_w);
    LT_REQUIRE(a->io_dtype == LT_BF16 || a->io_dtype == LT_F32, "io_dtype must be bf16 or f32");
    LT_REQUIRE(B <= e->cfg.max_batch, "lt_sample_views_guided: batch %d exceeds max_batch %d", B, e->cfg.max_batch);
    if (check_latent(e, "lt_sample_views_guided", a->latent_h, a->latent_w)) return 2;
    const int ncalls = (n_grid - 1) * 2;
    for (int i = 0; i < ncalls * 4; ++i)
        LT_REQUIRE(std::isfinite(coef_host[i]), "lt_sample_views_guided: coefficient %d of stage %d (interval %d) is not finite", i % 4, (i / 4) % 2, i / 8);
    LT_REQUIRE(e->reg_Y == 0 && e->prompt_B == B, "lt_prepare_prompt was called for batch %d, step has batch %d (multi-view sampling needs the V view "
               "prompts followed by V rows of the negative prompt)", e->prompt_B, B);
    {  // the model's own refusal of this shape, before anything is copied (no partial result)
        const int p = e->cfg.patch_size;
        float unused;
        if (softmax_scale_for(e, a, (a->latent_h / p) * (a->latent_w / p), &unused)) return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool bf = a->io_dtype == LT_BF16;
    float* tp = e->times.begin(ncalls * B, s);
    if (!tp) return 1;
    // generate.py:232-237, :253: t0, t1 are Python floats (the fp32 grid's values as doubles); dt, half_dt and t_mid = t0 + half_dt are doubles;
    // dt / half_dt multiply a tensor as fp32 scalars, the stage times are torch.full((2,), t0) and torch.full((2,), t_mid): fp32 of the double
    std::vector<float> dts(n_grid - 1), hdts(n_grid - 1);
    for (int i = 0; i + 1 < n_grid; ++i) {
        const double t0 = tgrid_host[i], dt = (double)tgrid_host[i + 1] - t0, half_dt = 0.5 * dt;
        dts[i] = (float)dt;
        hdts[i] = (float)half_dt;
        const float ts[2] = {(float)t0, (float)(t0 + half_dt)};
        for (int k = 0; k < 2; ++k)
            for (int b = 0; b < B; ++b) tp[((size_t)i * 2 + k) * B + b] = ts[k];
    }
    if (e->times.commit(ncalls * B, s)) return 1;
    Trajectory tr{e, a, 1, s, (size_t)C * HW * (bf ? 2 : 4)};
    if (tr.start(z_dev, traj_dev, true)) return 1;
    const int dt_code = bf ? 1 : 0;
    for (int i = 0; i + 1 < n_grid; ++i) {
        void *y0 = tr.y0(), *y1 = tr.y1();
        const int c0 = i * 2;
        const float* coef = coef_host + (size_t)i * 8;
        if (launch_views_guided_gather(y0, guidance_dev, noise_dev, e->vw_perm, e->vw_vsign, e->vw_isign, nullptr, e->ymid, 0.f, coef, V, C, HW, dt_code, s))
            return 1;
        if (tr.eval(e->ymid, c0, e->kbuf[0])) return 1;
        if (launch_views_guided_gather(y0, guidance_dev, noise_dev, e->vw_perm, e->vw_vsign, e->vw_isign, e->kbuf[0], e->ymid, hdts[i], coef + 4, V, C, HW,
                                       dt_code, s))
            return 1;
        if (tr.eval(e->ymid, c0 + 1, e->kbuf[1])) return 1;
        if (launch_views_reduce(y0, e->kbuf[1], e->vw_iperm, e->vw_isign, y1, dts[i], V, C, HW, dt_code, s)) return 1;
        if (tr.advance(i + 1)) return 1;
    }
    return tr.finish(final_dev);
}

// ---- SDE sampling (sde.hip) --------------------------------------------------------------------------------------------------------
extern "C" int lt_sample_sde(lt_engine* e, const void* z_dev, const void* noise_dev, void* traj_dev, void* final_dev, const float* steps_host,
                             int32_t n_steps, int32_t method, int32_t last_step, const float* last_coef_host, int32_t use_cfg,
                             const lt_step_args* a, void* stream) {
    LT_REQUIRE(e && z_dev && noise_dev && steps_host && a, "lt_sample_sde: null argument");
    if (refuse_if_capturing((hipStream_t)stream, "lt_sample_sde")) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(n_steps >= 2, "lt_sample_sde: n_steps %d (need at least 2: one loop step and the last step)", n_steps);
    LT_REQUIRE(method == LT_SDE_EULER || method == LT_SDE_HEUN, "lt_sample_sde: unknown method %d", method);
    LT_REQUIRE(last_step >= LT_SDE_LAST_NONE && last_step <= LT_SDE_LAST_EULER, "lt_sample_sde: unknown last_step %d", last_step);
    LT_REQUIRE(last_step == LT_SDE_LAST_NONE || (last_coef_host && final_dev), "lt_sample_sde: null argument (a last step needs last_coef_host and "
               "final_dev)");
    hipStream_t s = (hipStream_t)stream;
    const int B = a->batch;
    if (check_step_shape(e, "lt_sample_sde", a)) return 2;
    const int stages = method == LT_SDE_EULER ? 1 : 2;
    const int nloop = n_steps - 1;
    const int nrec = nloop * stages;
    const int has_last = last_step != LT_SDE_LAST_NONE;
    const int ncalls = nrec + has_last;
    // the score divides by var = sigma^2 - r sigma' sigma (path.py: get_score_from_velocity); the last-step rule Euler has no score
    for (int i = 0; i < nrec; ++i) {
        const float var = steps_host[(size_t)i * LT_SDE_REC + 2];
        LT_REQUIRE(std::isfinite(var) && var > 0.f, "lt_sample_sde: var %g of stage %d (step %d) is not finite and positive", (double)var, i % stages,
                   i / stages);
    }
    if (last_step == LT_SDE_LAST_MEAN || last_step == LT_SDE_LAST_TWEEDIE)
        LT_REQUIRE(std::isfinite(last_coef_host[2]) && last_coef_host[2] > 0.f, "lt_sample_sde: var %g of the last step is not finite and positive",
                   (double)last_coef_host[2]);
    const long long n = (long long)B * e->cfg.in_channels * a->latent_h * a->latent_w;
    const bool bf = a->io_dtype == LT_BF16;
    const size_t sbytes = (size_t)n * (bf ? 2 : 4);
    float* tp = e->times.begin(ncalls * B, s);
    if (!tp) return 1;
    // stage times: the loop hands the model a [B] vector of the state dtype (integrators.py: th.ones(B).to(x) * t), the last step an fp32 one
    for (int i = 0; i < ncalls; ++i) {
        const float tv = i < nrec ? steps_host[(size_t)i * LT_SDE_REC] : last_coef_host[0];
        for (int b = 0; b < B; ++b) tp[(size_t)i * B + b] = tv;
    }
    if (e->times.commit(ncalls * B, s)) return 1;
    Trajectory tr{e, a, use_cfg, s, sbytes};
    if (tr.start(z_dev, traj_dev, false)) return 1;  // the record holds loop state i in slot i: z is not part of it
    const int dt_code = bf ? 1 : 0;
    for (int i = 0; i < nloop; ++i) {
        void *y0 = tr.y0(), *y1 = tr.y1();
        const void* w = (const char*)noise_dev + (size_t)i * sbytes;
        const float* rec = steps_host + (size_t)i * stages * LT_SDE_REC;
        const int c0 = i * stages;
        if (method == LT_SDE_EULER) {
            if (tr.eval(y0, c0, e->kbuf[0])) return 1;
            if (launch_sde_step(LT_SDE_OP_EULER, y0, e->kbuf[0], w, nullptr, nullptr, y1, nullptr, rec, n, dt_code, s)) return 1;
        } else {  // xhat in ymid, K1 in kbuf[1], the predictor state in kbuf[2]
            if (launch_sde_step(LT_SDE_OP_HEUN_XHAT, y0, nullptr, w, nullptr, nullptr, e->ymid, nullptr, rec, n, dt_code, s)) return 1;
            if (tr.eval(e->ymid, c0, e->kbuf[0])) return 1;
            if (launch_sde_step(LT_SDE_OP_HEUN_K1, e->ymid, e->kbuf[0], nullptr, nullptr, nullptr, e->kbuf[2], e->kbuf[1], rec, n, dt_code, s)) return 1;
            if (tr.eval(e->kbuf[2], c0 + 1, e->kbuf[3])) return 1;
            if (launch_sde_step(LT_SDE_OP_HEUN_OUT, e->ymid, e->kbuf[3], nullptr, e->kbuf[1], e->kbuf[2], y1, nullptr, rec + LT_SDE_REC, n, dt_code, s))
                return 1;
        }
        if (tr.advance(i)) return 1;
    }
    if (has_last) {  // the last step's kernel writes final_dev itself
        const int op = last_step == LT_SDE_LAST_MEAN ? LT_SDE_OP_LAST_MEAN : (last_step == LT_SDE_LAST_TWEEDIE ? LT_SDE_OP_LAST_TWEEDIE : LT_SDE_OP_LAST_EULER);
        if (tr.eval(tr.y0(), nrec, e->kbuf[0])) return 1;
        if (launch_sde_step(op, tr.y0(), e->kbuf[0], nullptr, nullptr, nullptr, final_dev, nullptr, last_coef_host, n, dt_code, s)) return 1;
    }
    return tr.finish(has_last ? nullptr : final_dev);
}

// ---- prompt-driven editing: FlowEdit's inversion-free rule (flowedit.hip; transport/edit.py: sample_flowedit is the definition) ----
// a->batch = 4 B' rows per evaluation - source, target and their two negative prompts - around a state of B' rows; one plain forward per
// interval, the guidance expression per branch in the combine kernel.  Everything is checked before the first copy
extern "C" int lt_sample_flowedit(lt_engine* e, const void* z_dev, const void* x_src_dev, const void* noise_dev, void* traj_dev, void* final_dev,
                                  const float* tgrid_host, const float* scales_host, int32_t n_grid, const lt_step_args* a, void* stream) {
    const char* who = "lt_sample_flowedit";
    LT_REQUIRE(e && z_dev && x_src_dev && noise_dev && tgrid_host && scales_host && a, "%s: null argument", who);
    if (refuse_if_capturing((hipStream_t)stream, who)) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(n_grid >= 2, "%s: need at least 2 grid points", who);
    LT_REQUIRE(a->batch >= 4 && a->batch % 4 == 0, "%s: batch %d is not a positive multiple of 4 (source, target and their two negative prompts per "
               "image)", who, a->batch);
    if (check_step_shape(e, who, a)) return 2;
    const int C = e->cfg.in_channels;
    LT_REQUIRE(a->cfg_channels >= 1 && a->cfg_channels <= C, "%s: cfg_channels %d outside 1..in_channels %d", who, a->cfg_channels, C);
    for (int i = 0; i < n_grid; ++i) LT_REQUIRE(std::isfinite(tgrid_host[i]), "%s: grid value %d is not finite", who, i);
    for (int i = 0; i < 2 * (n_grid - 1); ++i)
        LT_REQUIRE(std::isfinite(scales_host[i]), "%s: the %s scale of interval %d is not finite", who, i % 2 ? "target" : "source", i / 2);
    LT_REQUIRE(e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): its captions belong to one cond and one uncond row, "
               "not to the four rows of an edit", who);
    LT_REQUIRE(e->prompt_B == a->batch, "%s: %s was called for batch %d, step has batch %d", who, e->v.labels ? "lt_prepare_labels" : "lt_prepare_prompt",
               e->prompt_B, a->batch);
    {  // the model's own refusal of this shape, before anything is copied (no partial result)
        const int p = e->cfg.patch_size;
        float unused;
        if (softmax_scale_for(e, a, (a->latent_h / p) * (a->latent_w / p), &unused)) return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int B = a->batch, Bp = B / 4, HW = a->latent_h * a->latent_w, ncalls = n_grid - 1;
    const long long n_half = (long long)Bp * C * HW;
    const bool bf = a->io_dtype == LT_BF16;
    const size_t sbytes = (size_t)n_half * (bf ? 2 : 4);
    float* tp = e->times.begin(ncalls * B, s);
    if (!tp) return 1;
    // the stage time handed to the model is the fp32 grid value, as in lt_sample_views (torch.full((4 B',), float(tgrid[i])))
    for (int i = 0; i < ncalls; ++i)
        for (int b = 0; b < B; ++b) tp[(size_t)i * B + b] = tgrid_host[i];
    if (e->times.commit(ncalls * B, s)) return 1;
    Trajectory tr{e, a, 0, s, sbytes};
    if (tr.start(z_dev, traj_dev, true)) return 1;
    const int dt_code = bf ? 1 : 0;
    for (int i = 0; i < ncalls; ++i) {
        // t, 1 - t and dt are Python floats in the host loop (the fp32 grid's values as doubles, 1 - t and t1 - t0 formed in double) that enter
        // torch's fp32 op-math
        const double t0 = tgrid_host[i];
        const float t = tgrid_host[i], omt = (float)(1.0 - t0), dt = (float)((double)tgrid_host[i + 1] - t0);
        const void* w = (const char*)noise_dev + (size_t)i * sbytes;
        if (launch_flowedit_mix(x_src_dev, tr.y0(), w, e->ymid, t, omt, n_half, dt_code, s)) return 1;
        if (tr.eval(e->ymid, i, e->kbuf[0])) return 1;
        if (launch_flowedit_combine(tr.y0(), e->kbuf[0], tr.y1(), scales_host[2 * i], scales_host[2 * i + 1], dt, Bp, C, HW, a->cfg_channels, dt_code, s))
            return 1;
        if (tr.advance(i + 1)) return 1;
    }
    return tr.finish(final_dev);
}

// ---- adaptive Runge-Kutta sampling (ode_adaptive.hip) ------------------------------------------------------------------------------
namespace {

// torchdiffeq's tableaus as transport/integrators.py states them (_TABLEAUS): the same double expressions, handed to the kernels as fp32
struct RkTableau {
    int stages, order;
    bool fsal;  // the last stage's state IS the solution (c_sol == the last beta row)
    double alpha[6], beta[6][6], c_sol[7], c_err[7], c_mid[7];
};
const RkTableau kRkTableaus[4] = {
    {6, 5, true,  // dopri5
     {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0},
     {{1.0 / 5},
      {3.0 / 40, 9.0 / 40},
      {44.0 / 45, -56.0 / 15, 32.0 / 9},
      {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
      {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656},
      {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}},
     {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0.0},
     {35.0 / 384 - 1951.0 / 21600, 0.0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720, -2187.0 / 6784 + 12231.0 / 42400,
      11.0 / 84 - 649.0 / 6300, -1.0 / 60},
     {6025192743.0 / 30085553152.0 / 2, 0.0, 51252292925.0 / 65400821598.0 / 2, -2691868925.0 / 45128329728.0 / 2,
      187940372067.0 / 1594534317056.0 / 2, -1776094331.0 / 19743644256.0 / 2, 11237099.0 / 235043384.0 / 2}},
    {3, 3, true,  // bosh3
     {1.0 / 2, 3.0 / 4, 1.0},
     {{1.0 / 2}, {0.0, 3.0 / 4}, {2.0 / 9, 1.0 / 3, 4.0 / 9}},
     {2.0 / 9, 1.0 / 3, 4.0 / 9, 0.0},
     {2.0 / 9 - 7.0 / 24, 1.0 / 3 - 1.0 / 4, 4.0 / 9 - 1.0 / 3, -1.0 / 8},
     {0.0, 0.5, 0.0, 0.0}},
    {2, 2, false,  // fehlberg2
     {1.0 / 2, 1.0},
     {{1.0 / 2}, {1.0 / 256, 255.0 / 256}},
     {1.0 / 512, 255.0 / 256, 1.0 / 512},
     {-1.0 / 512, 0.0, 1.0 / 512},
     {0.0, 0.5, 0.0}},
    {1, 2, false,  // adaptive_heun
     {1.0},
     {{1.0}},
     {0.5, 0.5},
     {0.5, -0.5},
     {0.5, 0.0}},
};

void to_f32(const double* c, int n, float* out) { for (int j = 0; j < n; ++j) out[j] = (float)c[j]; }

}  // namespace

extern "C" int lt_sample_ode_adaptive(lt_engine* e, const void* z_dev, void* traj_dev, const float* tgrid_host, int32_t n_grid, int32_t method,
                                      float rtol, float atol, float first_step, int32_t max_steps, int32_t use_cfg, int32_t t_round,
                                      const lt_step_args* a, void* stream, lt_ode_adaptive_stats* stats) {
#pragma clang fp contract(off)
    LT_REQUIRE(e && z_dev && traj_dev && tgrid_host && a, "lt_sample_ode_adaptive: null argument");
    if (refuse_if_capturing((hipStream_t)stream, "lt_sample_ode_adaptive")) return 2;  // (the host reads an error norm at every step)
    LtOptScope opt_scope(&e->opts);
    LT_REQUIRE(method >= LT_ODE_DOPRI5 && method <= LT_ODE_ADAPTIVE_HEUN, "lt_sample_ode_adaptive: unknown method %d", method);
    LT_REQUIRE(std::isfinite(rtol) && rtol > 0.f && std::isfinite(atol) && atol > 0.f,
               "lt_sample_ode_adaptive: rtol %g and atol %g must be finite and positive", (double)rtol, (double)atol);
    LT_REQUIRE(std::isfinite(first_step) && first_step >= 0.f, "lt_sample_ode_adaptive: first_step %g must be finite and >= 0", (double)first_step);
    LT_REQUIRE(max_steps >= 1, "lt_sample_ode_adaptive: max_steps %d (need at least 1)", max_steps);
    LT_REQUIRE(n_grid >= 2, "lt_sample_ode_adaptive: need at least 2 grid points");
    for (int i = 0; i + 1 < n_grid; ++i)
        LT_REQUIRE(std::isfinite(tgrid_host[i]) && std::isfinite(tgrid_host[i + 1]) && tgrid_host[i + 1] > tgrid_host[i],
                   "lt_sample_ode_adaptive: the grid is not strictly increasing at point %d (%g, then %g)", i, (double)tgrid_host[i],
                   (double)tgrid_host[i + 1]);
    hipStream_t s = (hipStream_t)stream;
    const int B = a->batch;
    if (check_step_shape(e, "lt_sample_ode_adaptive", a)) return 2;
    const RkTableau& T = kRkTableaus[method - LT_ODE_DOPRI5];
    const int S = T.stages;
    const long long n = (long long)B * e->cfg.in_channels * a->latent_h * a->latent_w;
    const bool bf = a->io_dtype == LT_BF16;
    const int dtc = bf ? 1 : 0;
    const size_t sbytes = (size_t)n * (bf ? 2 : 4);
    if (e->rk.reserve((size_t)e->cfg.max_batch * e->cfg.in_channels * e->cfg.max_tokens * e->cfg.patch_size * e->cfg.patch_size * sizeof(float))) {
        e->rk.release();
        return 1;
    }
    RkWork& W = e->rk;
    void* kp[LT_RK_MAX_SLOPES] = {e->kbuf[0], e->kbuf[1], e->kbuf[2], e->kbuf[3], W.k[0], W.k[1], W.k[2]};  // kp[0] = f(tcur, y)
    float beta[6][LT_RK_MAX_SLOPES], c_sol[LT_RK_MAX_SLOPES], c_err[LT_RK_MAX_SLOPES], c_mid[LT_RK_MAX_SLOPES];
    for (int i = 0; i < S; ++i) to_f32(T.beta[i], i + 1, beta[i]);
    to_f32(T.c_sol, S + 1, c_sol);
    to_f32(T.c_err, S + 1, c_err);
    to_f32(T.c_mid, S + 1, c_mid);

    Trajectory tr{e, a, use_cfg, s, sbytes};
    // `count` stage times for the evaluations that follow (the stream is idle: every round below ends with a synchronisation)
    auto send_times = [&](const float* ts, int count) -> int {
        float* tp = e->times.begin(count * B, s);
        if (!tp) return 1;
        for (int k = 0; k < count; ++k) {
            const float tv = (t_round && bf) ? bf16_round_host(ts[k]) : ts[k];
            for (int b = 0; b < B; ++b) tp[(size_t)k * B + b] = tv;
        }
        return e->times.commit(count * B, s);
    };
    // the host reads `count` norms: the one synchronisation of a round
    auto read_norms = [&](int count) -> int {
        LT_CHECK_HIP(hipMemcpyAsync(W.norm_host, W.norm_dev, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, s));
        LT_CHECK_HIP(hipStreamSynchronize(s));
        return 0;
    };
    auto const_k = [&]() { return (const void* const*)kp; };

    if (tr.start(z_dev, traj_dev, true)) return 1;
    float tcur = tgrid_host[0], tprev = tcur;
    if (send_times(&tcur, 1)) return 1;
    if (tr.eval(tr.y0(), 0, kp[0])) return 1;
    float dt = first_step;
    if (!(first_step > 0.f)) {  // torchdiffeq's _select_initial_step (integrators.py:150-162)
        if (launch_rms_norm(tr.y0(), nullptr, tr.y0(), rtol, atol, nullptr, W.ws, W.norm_dev, n, dtc, s)) return 1;
        if (launch_rms_norm(kp[0], nullptr, tr.y0(), rtol, atol, nullptr, W.ws, W.norm_dev + 1, n, dtc, s)) return 1;
        if (read_norms(2)) return 1;
        const float d0 = W.norm_host[0], d1 = W.norm_host[1];
        const float h0 = ((double)d0 >= 1e-5 && (double)d1 >= 1e-5) ? (0.01f * d0) / d1 : 1e-6f;
        const float th = tcur + h0;
        const float one = 1.f;
        if (send_times(&th, 1)) return 1;
        if (launch_rk_stage(tr.y0(), const_k(), &one, 1, h0, e->ymid, n, dtc, s)) return 1;
        if (tr.eval(e->ymid, 0, kp[1])) return 1;
        if (launch_rms_norm(kp[1], kp[0], tr.y0(), rtol, atol, nullptr, W.ws, W.norm_dev, n, dtc, s)) return 1;
        if (read_norms(1)) return 1;
        const float d2 = W.norm_host[0] / h0;
        float h1;
        if ((double)d1 <= 1e-15 && (double)d2 <= 1e-15) {
            h1 = std::max(1e-6f, h0 * 1e-3f);
        } else {
            const float base = (1.f / std::max(d1, d2)) * 0.01f;  // 0.01 / tensor is reciprocal(tensor) * 0.01 in torch
            h1 = (float)std::pow((double)base, 1.0 / (double)T.order);
        }
        dt = std::min(100.f * h0, h1);
        LT_REQUIRE(std::isfinite(dt) && dt > 0.f, "lt_sample_ode_adaptive: the initial step heuristic gave dt = %g (norms %g, %g, %g): the model "
                   "output is not finite", (double)dt, (double)d0, (double)d1, (double)d2);
    }
    const float dt_first = dt;
    int accepted = 0, rejected = 0, attempts = 0;
    const void* cf[5] = {nullptr, W.coef[0], W.coef[1], W.coef[2], W.coef[3]};  // dense output of the last accepted step with a grid point in it
    for (int gi = 1; gi < n_grid; ++gi) {
        const float next_t = tgrid_host[gi];
        int steps = 0;
        while (next_t > tcur) {
            LT_REQUIRE(steps < max_steps, "lt_sample_ode_adaptive: max_steps %d exceeded between grid points %d and %d (t = %g, dt = %g)", max_steps,
                       gi - 1, gi, (double)tcur, (double)dt);
            ++steps;
            const float t1 = tcur + dt;
            LT_REQUIRE(t1 > tcur, "lt_sample_ode_adaptive: step size underflow (t = %g, dt = %g)", (double)tcur, (double)dt);
            if (stats && stats->dt_host && attempts < stats->dt_cap) stats->dt_host[attempts] = dt;
            ++attempts;
            float ts[6];
            for (int i = 0; i < S; ++i) ts[i] = T.alpha[i] == 1.0 ? t1 : tcur + (float)T.alpha[i] * dt;
            if (send_times(ts, S)) return 1;
            void *y = tr.y0(), *y1 = tr.y1();
            for (int i = 0; i < S; ++i) {
                void* yi = (T.fsal && i == S - 1) ? y1 : e->ymid;
                if (launch_rk_stage(y, const_k(), beta[i], i + 1, dt, yi, n, dtc, s)) return 1;
                if (tr.eval(yi, i, kp[i + 1])) return 1;
            }
            if (!T.fsal && launch_rk_stage(y, const_k(), c_sol, S + 1, dt, y1, n, dtc, s)) return 1;
            if (launch_rk_error_norm(y, y1, const_k(), c_err, S + 1, dt, rtol, atol, nullptr, W.ws, W.norm_dev, n, dtc, s)) return 1;
            if (read_norms(1)) return 1;
            const double ratio = (double)W.norm_host[0];
            LT_REQUIRE(std::isfinite(ratio), "lt_sample_ode_adaptive: the error ratio of the step at t = %g, dt = %g is not finite", (double)tcur,
                       (double)dt);
            if (ratio <= 1.0) {
                if (next_t <= t1) {  // a grid point lies in this step: its dense output (a step without one is never interpolated)
                    if (launch_rk_stage(y, const_k(), c_mid, S + 1, dt, e->ymid, n, dtc, s)) return 1;
                    if (launch_rk_dense(y, y1, e->ymid, kp[0], kp[S], dt, W.coef[0], W.coef[1], W.coef[2], W.coef[3], n, dtc, s)) return 1;
                    cf[0] = y;  // (stays intact until the next attempted step writes its y1 there)
                }
                tprev = tcur;
                tcur = t1;
                tr.cur ^= 1;
                std::swap(kp[0], kp[S]);  // like torchdiffeq, the last stage's slope stands in for f(t1, y1) whatever the tableau
                ++accepted;
            } else {
                ++rejected;
            }
            // _optimal_step_size(dt, ratio, safety 0.9, ifactor 10, dfactor 0.2, order): the factor in double, dt in fp32
            double factor = 10.0;
            if (ratio != 0.0) {
                const double dfactor = ratio < 1.0 ? 1.0 : 0.2;
                factor = std::min(10.0, std::max(0.9 / std::pow(ratio, 1.0 / (double)T.order), dfactor));
            }
            dt = dt * (float)factor;
        }
        const float x = (next_t - tprev) / (tcur - tprev);  // _interp_evaluate
        if (launch_rk_interp(cf, x, (char*)traj_dev + (size_t)gi * sbytes, n, dtc, s)) return 1;
    }
    if (stats) {
        stats->nfe = tr.nfe;
        stats->accepted = accepted;
        stats->rejected = rejected;
        stats->first_step = dt_first;
        stats->dt_count = attempts;
    }
    return tr.finish(nullptr);
}

extern "C" int64_t lt_last_nfe(lt_engine* e) { return e ? e->last_nfe : -1; }
extern "C" int64_t lt_last_eval_rows(lt_engine* e) { return e ? e->last_eval_rows : -1; }
extern "C" int lt_debug_cache_read(lt_engine* e, int32_t which, void* dst_dev, int64_t n, void* stream) {
    LT_REQUIRE(e && dst_dev, "lt_debug_cache_read: null argument");
    LT_REQUIRE(e->c_sums_host, "lt_debug_cache_read: the step-cache buffers are not allocated yet");
    const u16* src[5] = {e->c_hprev, e->c_x0, e->c_r, e->x, e->h};
    LT_REQUIRE(which >= 0 && which < 5, "lt_debug_cache_read: which %d outside 0..4", which);
    LT_REQUIRE(n > 0 && n <= (int64_t)e->cfg.max_batch * e->cfg.max_tokens * e->d, "lt_debug_cache_read: %lld words outside the buffer", (long long)n);
    LT_CHECK_HIP(hipMemcpyAsync(dst_dev, src[which], (size_t)n * sizeof(u16), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
extern "C" int64_t lt_last_cache_hits(lt_engine* e) { return e ? e->last_cache_hits : -1; }

// ---- tiled (MultiDiffusion) sampling: one canvas latent, the model on overlapping windows of it, their predictions fused ------
void drop_windows(lt_engine* e) {
    if (e->tw_weight) (void)hipFree(e->tw_weight);
    if (e->tw_wsum) (void)hipFree(e->tw_wsum);
    if (e->tw_bad) (void)hipFree(e->tw_bad);
    if (e->tw_in) (void)hipFree(e->tw_in);
    if (e->tw_out) (void)hipFree(e->tw_out);
    e->tw_weight = e->tw_wsum = nullptr; e->tw_bad = nullptr; e->tw_in = e->tw_out = nullptr;
    e->tw.n = 0;
}

// the buffers of the tiled calls, allocated once at their largest size (engine.h); the composed calls use the two row buffers
static int ensure_window_buffers(lt_engine* e, const char* who) {
    if (e->tw_out) return 0;
    const lt_config& c = e->cfg;
    const size_t win_px = (size_t)c.max_tokens * c.patch_size * c.patch_size, rows = (size_t)c.max_batch * c.in_channels * win_px * sizeof(float);
    if (hipMalloc((void**)&e->tw_weight, win_px * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&e->tw_wsum, (size_t)((c.max_batch + 1) / 2) * win_px * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&e->tw_bad, sizeof(int)) != hipSuccess || hipMalloc(&e->tw_in, rows) != hipSuccess ||
        hipMalloc(&e->tw_out, rows) != hipSuccess) {
        drop_windows(e);
        lt_set_error("%s: out of device memory for the window buffers", who);
        return 1;
    }
    return 0;
}

extern "C" int lt_set_windows(lt_engine* e, const int32_t* offsets_host, int32_t n, int32_t win_h, int32_t win_w, int32_t canvas_h, int32_t canvas_w,
                              const float* weight_dev, void* stream) {
    const char* who = "lt_set_windows";
    LT_REQUIRE(e, "%s: null engine", who);
    hipStream_t s = (hipStream_t)stream;
    if (refuse_if_capturing(s, who)) return 2;  // (allocates, synchronises)
    const lt_config& c = e->cfg;
    if (n == 0) {  // drop the table (the buffers stay: a graph the caller recorded may hold them)
        LT_CHECK_HIP(hipStreamSynchronize(s));
        e->tw.n = 0;
        return 0;
    }
    LT_REQUIRE(offsets_host, "%s: null argument (offsets_host: n rows of (top, left))", who);
    LT_REQUIRE(n >= 1 && n <= LT_WINDOWS_MAX, "%s: n = %d windows (1 .. %d; 0 drops the table)", who, n, LT_WINDOWS_MAX);
    LT_REQUIRE(2 * (long long)n <= c.max_batch, "%s: %d windows need a batch of 2 n = %d rows (window prompts + negative prompts), max_batch is %d", who,
               n, 2 * n, c.max_batch);
    const int p = c.patch_size;
    LT_REQUIRE(win_h > 0 && win_w > 0 && canvas_h > 0 && canvas_w > 0 && win_h % p == 0 && win_w % p == 0 && canvas_h % p == 0 && canvas_w % p == 0,
               "%s: window %dx%d / canvas %dx%d: sizes must be positive multiples of the patch size %d", who, win_h, win_w, canvas_h, canvas_w, p);
    for (int k = 0; k < n; ++k)
        LT_REQUIRE(offsets_host[2 * k] % p == 0 && offsets_host[2 * k + 1] % p == 0, "%s: the offset (%d, %d) of window %d is not a multiple of the "
                   "patch size %d", who, offsets_host[2 * k], offsets_host[2 * k + 1], k, p);
    WindowTable t;
    if (window_table_build(who, offsets_host, n, win_h, win_w, canvas_h, canvas_w, &t)) return 2;  // (every window inside the canvas)
    const int hp = win_h / p, wp = win_w / p, wrow = e->v.eol ? wp + 1 : wp;
    LT_REQUIRE((long long)hp * wrow <= c.max_tokens, "%s: a window of %dx%d has %d latent tokens, max_tokens is %d", who, win_h, win_w, hp * wrow,
               c.max_tokens);
    LT_REQUIRE(e->v.rope_1d ? hp * wrow <= e->rope_len : (hp <= e->rope_len && wp <= e->rope_len),
               "%s: a window grid of %dx%d tokens exceeds the RoPE table (%d)", who, hp, wp, e->rope_len);
    // a covered canvas has no more pixels than its windows: the bound that keeps the cover kernel inside the sums (and the canvas inside the
    // state buffers, lumina_dit.h)
    LT_REQUIRE((long long)canvas_h * canvas_w <= (long long)n * win_h * win_w, "%s: a canvas of %dx%d cannot be covered by %d windows of %dx%d", who,
               canvas_h, canvas_w, n, win_h, win_w);
    if (ensure_window_buffers(e, who)) return 1;
    // the sums are formed in e->tw_out, which no call is using, from the caller's weights: a refused table leaves the one in force as it was
    int bad = -1;
    if (launch_windows_cover(t, weight_dev, (float*)e->tw_out, e->tw_bad, s)) return 1;
    LT_CHECK_HIP(hipMemcpyAsync(&bad, e->tw_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    LT_CHECK_HIP(hipStreamSynchronize(s));  // (also: no kernel of an earlier call still reads the tables that are rewritten below)
    LT_REQUIRE(bad == 0, "%s: the canvas is not covered: %d of its %d pixels lie under no window, or under weights whose sum is not finite and "
               "above 0", who, bad, canvas_h * canvas_w);
    LT_CHECK_HIP(hipMemcpyAsync(e->tw_wsum, e->tw_out, (size_t)canvas_h * canvas_w * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (weight_dev) LT_CHECK_HIP(hipMemcpyAsync(e->tw_weight, weight_dev, (size_t)win_h * win_w * sizeof(float), hipMemcpyDeviceToDevice, s));
    e->tw = t;
    e->tw_has_weight = weight_dev != nullptr;
    return 0;
}

namespace {
// what both tiled evaluation entries refuse, by name, before anything is launched
int check_tiled_call(const lt_engine* e, const char* who, const lt_step_args* a) {
    LT_REQUIRE(e->tw.n >= 1, "%s: no window table (call lt_set_windows first)", who);
    const int n = e->tw.n;
    LT_REQUIRE(a->batch == 2 * n, "%s: %d windows need a->batch = 2 n = %d (window prompts + negative prompts), got %d", who, n, 2 * n, a->batch);
    LT_REQUIRE(a->latent_h == e->tw.win_h && a->latent_w == e->tw.win_w, "%s: the window table is for windows of %dx%d, the call has a latent of %dx%d",
               who, e->tw.win_h, e->tw.win_w, a->latent_h, a->latent_w);
    LT_REQUIRE(a->io_dtype == LT_BF16 || a->io_dtype == LT_F32, "io_dtype must be bf16 or f32");
    LT_REQUIRE(e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): its captions belong to one image, not to a row per "
               "window", who);
    LT_REQUIRE(e->skip.empty() && e->perturb.empty(), "%s: a layer-skip or perturb set is not served", who);
    LT_REQUIRE(e->prompt_B == 2 * n, "%s: %s was called for batch %d, %d windows need %d rows (the window prompts, then the negative prompts)", who,
               e->v.labels ? "lt_prepare_labels" : "lt_prepare_prompt", e->prompt_B, n, 2 * n);
    return 0;
}
}  // namespace

extern "C" int lt_forward_tiled(lt_engine* e, const void* y_dev, const float* t_dev, void* v_dev, const lt_step_args* a, void* stream) {
    const char* who = "lt_forward_tiled";
    LT_REQUIRE(e && y_dev && t_dev && v_dev && a, "%s: null argument", who);
    hipStream_t s = (hipStream_t)stream;
    LtOptScope opt_scope(&e->opts);
    if (check_tiled_call(e, who, a)) return 2;
    const int C = e->cfg.in_channels, dt_code = a->io_dtype == LT_BF16 ? 1 : 0;
    if (launch_windows_gather(y_dev, e->tw, e->tw_in, C, dt_code, s)) return 1;
    if (int rc = forward_graphed(e, e->tw_in, t_dev, e->tw_out, a, 1, s)) return rc;
    return launch_windows_reduce(e->tw_out, e->tw, e->tw_has_weight ? e->tw_weight : nullptr, e->tw_wsum, v_dev, C, dt_code, s);
}

extern "C" int lt_sample_ode_tiled(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                   int32_t method, int32_t t_round, const lt_step_args* a, void* stream) {
    const char* who = "lt_sample_ode_tiled";
    LT_REQUIRE(e && z_dev && tgrid_host && a, "%s: null argument", who);
    if (refuse_if_capturing((hipStream_t)stream, who)) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    if (check_grid_method(who, n_grid, method, false, " (tiled sampling serves the fixed-grid methods euler, midpoint, rk4)")) return 2;
    if (check_tiled_call(e, who, a)) return 2;
    GridCall c{z_dev, traj_dev, final_dev, tgrid_host, n_grid, 1, t_round, a, (hipStream_t)stream,
               (long long)e->cfg.in_channels * e->tw.canvas_h * e->tw.canvas_w, nullptr, method};
    c.tiled = true;
    return ode_fixed_grid(e, c, {}, nullptr);
}

// ---- composed guidance: K weighted prompts and one base prompt per image (compose.hip; transport/guidance.py: guided_compose /
// sample_cfg_compose are the definition).  a->batch = (K + 1) B' rows per evaluation around a state of B' rows; the evaluation is a plain
// forward (LT_KIND_WHOLE, use_cfg = 0) under the graph key an lt_forward of that shape has, the two kernels run outside the graph -----------
namespace {
// what both composed entries refuse, by name, before anything is launched
int check_compose_call(lt_engine* e, const char* who, const lt_step_args* a, const float* w_host, int K, int rows_of_weights) {
    LT_REQUIRE(K >= 1 && K <= LT_COMPOSE_MAX, "%s: K = %d prompts (1 .. %d)", who, K, LT_COMPOSE_MAX);
    LT_REQUIRE(a->batch >= K + 1 && a->batch % (K + 1) == 0, "%s: batch %d is not a positive multiple of K + 1 = %d (K prompt rows and the base row per "
               "image)", who, a->batch, K + 1);
    if (check_step_shape(e, who, a)) return 2;
    for (int i = 0; i < rows_of_weights * K; ++i)
        LT_REQUIRE(std::isfinite(w_host[i]), "%s: the weight of prompt %d at evaluation %d is not finite", who, i % K, i / K);
    LT_REQUIRE(a->cfg_channels >= 1 && a->cfg_channels <= e->cfg.in_channels, "%s: cfg_channels %d outside 1..in_channels %d", who, a->cfg_channels,
               e->cfg.in_channels);
    LT_REQUIRE(e->reg_Y == 0, "%s: a regional prompt is prepared (lt_prepare_prompt_regional): its captions belong to one cond and one uncond row, "
               "not to the K + 1 rows of a composition", who);
    LT_REQUIRE(e->skip.empty() && e->perturb.empty(), "%s: a layer-skip or perturb set is not served", who);
    LT_REQUIRE(e->prompt_B == a->batch, "%s: %s was called for batch %d, step has batch %d", who, e->v.labels ? "lt_prepare_labels" : "lt_prepare_prompt",
               e->prompt_B, a->batch);
    {  // the model's own refusal of this shape, before anything is copied (no partial result)
        const int p = e->cfg.patch_size;
        float unused;
        if (softmax_scale_for(e, a, (a->latent_h / p) * (a->latent_w / p), &unused)) return 1;
    }
    return 0;
}
}  // namespace

extern "C" int lt_forward_compose(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const float* w_host, int32_t K,
                                  const lt_step_args* a, void* stream) {
    const char* who = "lt_forward_compose";
    LT_REQUIRE(e && x_dev && t_dev && out_dev && w_host && a, "%s: null argument", who);
    hipStream_t s = (hipStream_t)stream;
    LtOptScope opt_scope(&e->opts);
    if (check_compose_call(e, who, a, w_host, K, 1)) return 2;
    if (!e->tw_out && refuse_if_capturing(s, who)) return 2;  // (the first composed or tiled call of an engine allocates the row buffers)
    if (ensure_window_buffers(e, who)) return 1;
    const int Bp = a->batch / (K + 1), C = e->cfg.in_channels, HW = a->latent_h * a->latent_w, dt_code = a->io_dtype == LT_BF16 ? 1 : 0;
    if (launch_compose_replicate(x_dev, e->tw_in, K, Bp, C, HW, dt_code, s)) return 1;
    if (int rc = forward_graphed(e, e->tw_in, t_dev, e->tw_out, a, 0, s)) return rc;
    return launch_compose_guidance(e->tw_out, out_dev, w_host, K, Bp, C, HW, a->cfg_channels, dt_code, s);
}

extern "C" int lt_sample_ode_compose(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                     int32_t method, const float* w_host, int32_t K, int32_t t_round, const lt_step_args* a, void* stream) {
    const char* who = "lt_sample_ode_compose";
    LT_REQUIRE(e && z_dev && tgrid_host && w_host && a, "%s: null argument", who);
    if (refuse_if_capturing((hipStream_t)stream, who)) return 2;  // (the stage times travel through a host staging buffer that the next call rewrites)
    LtOptScope opt_scope(&e->opts);
    if (check_grid_method(who, n_grid, method, false, " (composed guidance serves the fixed-grid methods euler, midpoint, rk4)")) return 2;
    const int stages = method == LT_ODE_EULER ? 1 : (method == LT_ODE_MIDPOINT ? 2 : 4);
    if (check_compose_call(e, who, a, w_host, K, (n_grid - 1) * stages)) return 2;
    if (ensure_window_buffers(e, who)) return 1;
    GridCall c{z_dev, traj_dev, final_dev, tgrid_host, n_grid, 0, t_round, a, (hipStream_t)stream, dense_elems(e, a) / (K + 1), nullptr, method};
    c.compose_K = K; c.compose_w = w_host;
    return ode_fixed_grid(e, c, {}, nullptr);
}
