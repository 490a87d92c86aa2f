// What the evaluations of one guided trajectory are (samplers.hip), decided once by the entry point: the form of the guidance, the host
// tables it reads, what travels behind the stage times in the committed buffer, and what evaluation number `call` issues.  Includes nothing
// of HIP, so that tests/host/guidance_plan.hip compiles it alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "eval_kind.h"

// Step caching (transport/cache.py: CacheController is the definition): the accumulator of one trajectory, in C++ doubles without
// contraction.  step() takes the indicator sums of an evaluation that is neither the first nor the last and says whether the stack runs
struct CacheControl {
    double thr = 0.0, c[5] = {0, 0, 0, 1, 0}, acc = 0.0;
    double* stats = nullptr;  // null, or ncalls x 3: rel, acc after the add, ran
    bool step(double s1, double s0, double* rel_out) {
#pragma clang fp contract(off)
        if (s0 == 0.0) { *rel_out = INFINITY; return true; }  // (nothing to compare with: the stack runs, the accumulator takes nothing)
        const double rel = s1 / s0;
        double p = c[0];
        for (int k = 1; k < 5; ++k) p = p * rel + c[k];
        acc += p;
        *rel_out = rel;
        return !(acc < thr);
    }
};

// The forms exclude each other: a trajectory has one.
enum LtGuidanceForm {
    LT_PLAN_NONE = 0,           // every evaluation whole, at the host's scale (a->cfg_scale under use_cfg)
    LT_PLAN_TABLE,              // a scale per evaluation (lt_sample_ode_cfg_schedule)
    LT_PLAN_RULE,               // ... under the rescale / norm-limit rule { rescale, norm limit } (lt_sample_ode_cfg_rule)
    LT_PLAN_REUSE,              // ... with a flag per evaluation: 0 take and store the cond - uncond difference, 1 reuse it
    LT_PLAN_SLG,                // ... with a scale s per evaluation and the layer sets of the degraded evaluation (slg / pag)
    LT_PLAN_PROJECT_APG,        // ... projected, with { eta, beta, r } and a momentum buffer (lt_sample_ode_cfg_project)
    LT_PLAN_PROJECT_ZERO_STAR,  // ... projected, CFG-Zero*: the three parameters unread, `zero_init` intervals of zero velocity at the start
    LT_PLAN_CACHED              // step caching: no table; the controller decides behind each head (lt_sample_ode_cached)
};
// the buffers an evaluation leaves behind for a later one, each with a signature in the engine: e->g_delta, e->p_mom, e->c_r
enum LtStoredBuffer { LT_STORED_NONE = 0, LT_STORED_DELTA, LT_STORED_MOMENTUM, LT_STORED_RESIDUAL };
// where the closing kind finds its guidance scale: nowhere (the host's), word `call` of the committed table, the engine's fixed words
enum LtScaleWord { LT_SCALE_HOST = 0, LT_SCALE_TABLE, LT_SCALE_FIXED };

// What one evaluation of the trajectory issues.  Two kinds: a skip-layer stage - the store under the layer sets (its scale in the fixed words),
// then the closing kind.  LT_KIND_CACHE_HEAD: a step-cached evaluation; what follows the head is the controller's choice at run time, and
// `rewrites` holds only if the stack runs.
struct GuidanceStep { LtEvalKind kinds[2]; int n_kinds; LtScaleWord scale; LtStoredBuffer rewrites; };

struct GuidancePlan {
    LtGuidanceForm form = LT_PLAN_NONE;
    const float* table = nullptr;    // host: one scale per evaluation (every form but none and cached)
    const float* rule = nullptr;     // LT_PLAN_RULE: { rescale, norm limit }
    const int32_t* reuse = nullptr;  // LT_PLAN_REUSE: one flag per evaluation
    const float* slg = nullptr;      // LT_PLAN_SLG: one scale s per evaluation; the blocks left out and the blocks perturbed;
    const int32_t *skip = nullptr, *perturb = nullptr; int n_skip = 0, n_perturb = 0;
    bool pag = false;                // ... the entry that takes both sets, either of which may be empty
    const int32_t* blur = nullptr; int n_blur = 0; float blur_sigma = 0.f;  // ... smoothed-energy guidance: the blocks run on blurred queries
    int project_form = 0;            // projected: the form as the caller passed it (checked behind the shape), { eta, beta, r }, and
    float par[3] = {0.f, 0.f, 0.f}; int zero_init = 0;  // ... the intervals of zero velocity at the start
    CacheControl* cache = nullptr;   // LT_PLAN_CACHED

    static GuidancePlan of_table(const float* table) { GuidancePlan p; p.form = LT_PLAN_TABLE; p.table = table; return p; }
    static GuidancePlan of_rule(const float* table, const float* rule) { GuidancePlan p = of_table(table); p.form = LT_PLAN_RULE; p.rule = rule; return p; }
    static GuidancePlan of_reuse(const float* table, const int32_t* flags) { GuidancePlan p = of_table(table); p.form = LT_PLAN_REUSE; p.reuse = flags; return p; }
    static GuidancePlan of_slg(const float* table, const float* slg, const int32_t* skip, int n_skip, const int32_t* perturb, int n_perturb, bool pag) {
        GuidancePlan p = of_table(table);
        p.form = LT_PLAN_SLG; p.slg = slg; p.skip = skip; p.n_skip = n_skip; p.perturb = perturb; p.n_perturb = n_perturb; p.pag = pag;
        return p;
    }
    static GuidancePlan of_seg(const float* table, const float* seg, const int32_t* skip, int n_skip, const int32_t* blur, int n_blur, float sigma) {
        GuidancePlan p = of_slg(table, seg, skip, n_skip, nullptr, 0, true);
        p.blur = blur; p.n_blur = n_blur; p.blur_sigma = sigma;
        return p;
    }
    static GuidancePlan of_project(const float* table, bool apg, int form_passed, float eta, float beta, float r, int zero_init) {
        GuidancePlan p = of_table(table);
        p.form = apg ? LT_PLAN_PROJECT_APG : LT_PLAN_PROJECT_ZERO_STAR;
        p.project_form = form_passed; p.par[0] = eta; p.par[1] = beta; p.par[2] = r; p.zero_init = zero_init;
        return p;
    }
    static GuidancePlan of_cache(CacheControl* cc) { GuidancePlan p; p.form = LT_PLAN_CACHED; p.cache = cc; return p; }

    bool has_table() const { return form != LT_PLAN_NONE && form != LT_PLAN_CACHED; }
    bool projected() const { return form == LT_PLAN_PROJECT_APG || form == LT_PLAN_PROJECT_ZERO_STAR; }

    // The committed buffer of a trajectory of `ncalls` evaluations on B rows: ncalls * B stage times, then the tail - the scale table, then the
    // form's second block (the rule pair, the s table or the projected triple).  Offsets in floats from the buffer's start
    int second_floats(int ncalls) const { return form == LT_PLAN_RULE ? 2 : form == LT_PLAN_SLG ? ncalls : projected() ? 3 : 0; }
    int tail_floats(int ncalls) const { return has_table() ? ncalls + second_floats(ncalls) : 0; }
    static size_t table_offset(int ncalls, int B) { return (size_t)ncalls * B; }
    static size_t second_offset(int ncalls, int B) { return table_offset(ncalls, B) + ncalls; }
    void fill_tail(float* behind_times, int ncalls) const {
        if (!has_table()) return;
        memcpy(behind_times, table, (size_t)ncalls * sizeof(float));
        const float* second = form == LT_PLAN_RULE ? rule : form == LT_PLAN_SLG ? slg : par;
        memcpy(behind_times + ncalls, second, (size_t)second_floats(ncalls) * sizeof(float));
    }

    GuidanceStep step_of(int call) const {
        if (form == LT_PLAN_CACHED) return {{LT_KIND_CACHE_HEAD, LT_KIND_COUNT}, 1, LT_SCALE_HOST, LT_STORED_RESIDUAL};
        if (!has_table()) return {{LT_KIND_WHOLE, LT_KIND_COUNT}, 1, LT_SCALE_HOST, LT_STORED_NONE};
        // scale 1 exactly: the guided output is the conditional one - the cond rows alone, written to both halves
        const bool cond_only = table[call] == 1.0f;
        if (form == LT_PLAN_REUSE && !cond_only)
            return reuse[call] != 0 ? GuidanceStep{{LT_KIND_REUSE_AGAIN, LT_KIND_COUNT}, 1, LT_SCALE_TABLE, LT_STORED_NONE}
                                    : GuidanceStep{{LT_KIND_REUSE_STORE, LT_KIND_COUNT}, 1, LT_SCALE_TABLE, LT_STORED_DELTA};
        if (form == LT_PLAN_SLG && slg[call] != 0.0f)  // (at s = 0 the stage is the schedule call's)
            return cond_only ? GuidanceStep{{LT_KIND_SLG_STORE, LT_KIND_SLG_COND}, 2, LT_SCALE_FIXED, LT_STORED_NONE}
                             : GuidanceStep{{LT_KIND_SLG_STORE, LT_KIND_SLG_GUIDED}, 2, LT_SCALE_TABLE, LT_STORED_NONE};
        // a guided evaluation under APG advances the momentum buffer
        if (!cond_only && form == LT_PLAN_PROJECT_APG) return {{LT_KIND_RULE, LT_KIND_COUNT}, 1, LT_SCALE_TABLE, LT_STORED_MOMENTUM};
        const LtEvalKind kind = cond_only ? LT_KIND_COND_ONLY : (form == LT_PLAN_RULE || projected()) ? LT_KIND_RULE : LT_KIND_DEV_GUIDED;
        return {{kind, LT_KIND_COUNT}, 1, LT_SCALE_TABLE, LT_STORED_NONE};
    }
};
