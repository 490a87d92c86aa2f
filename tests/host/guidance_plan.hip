// Host only: the plan of a guided trajectory (csrc/guidance_plan.h) against the rules the samplers applied before the plan existed, written
// out here literally as they stood in Trajectory::eval, ode_fixed_grid and ode_multistep - plain ifs over nullable pointers, not a copy of
// step_of.  Its own main; links nothing of the engine.
#include <cmath>
#include <cstdio>
#include <vector>

#include "guidance_plan.h"

static int failures = 0;
static void fail(const char* form, int call, const char* what, int got, int want) {
    std::printf("%s, call %d: %s is %d, the rule says %d\n", form, call, what, got, want);
    ++failures;
}

// the optional members of the former Trajectory and of the former CfgSchedule
struct Old {
    bool cache = false;
    const float* cfg_host = nullptr;
    bool cfg_rule = false;     // cs->rule != nullptr || cs->project != nullptr
    int rule_form = 0;         // e->rule_form under ProjectScope: 0, 1 (APG), 2 (CFG-Zero*)
    const int32_t* reuse_host = nullptr;
    const float* slg_host = nullptr;
    const float *rule = nullptr, *project = nullptr;  // what travelled behind the scales
};

// Trajectory::eval and the eval_* it chose, as they stood: the kinds issued, where the closing one read its scale, what it rewrote
static GuidanceStep old_eval(const Old& o, int call) {
    if (o.cache) return {{LT_KIND_CACHE_HEAD, LT_KIND_COUNT}, 1, LT_SCALE_HOST, LT_STORED_RESIDUAL};  // eval_cached: the head; c_r if the stack runs
    if (!o.cfg_host) return {{LT_KIND_WHOLE, LT_KIND_COUNT}, 1, LT_SCALE_HOST, LT_STORED_NONE};
    const bool cond_only = o.cfg_host[call] == 1.0f;
    if (o.reuse_host && !cond_only) {  // eval_reuse: cfg_dev + call
        const bool again = o.reuse_host[call] != 0;
        return {{again ? LT_KIND_REUSE_AGAIN : LT_KIND_REUSE_STORE, LT_KIND_COUNT}, 1, LT_SCALE_TABLE, again ? LT_STORED_NONE : LT_STORED_DELTA};
    }
    if (o.slg_host && o.slg_host[call] != 0.0f)  // eval_slg: the store at e->g_cfg, then cond at e->g_cfg or guided at cfg_dev + call
        return {{LT_KIND_SLG_STORE, cond_only ? LT_KIND_SLG_COND : LT_KIND_SLG_GUIDED}, 2, cond_only ? LT_SCALE_FIXED : LT_SCALE_TABLE, LT_STORED_NONE};
    if (!cond_only && o.cfg_rule && o.rule_form == 1) return {{LT_KIND_RULE, LT_KIND_COUNT}, 1, LT_SCALE_TABLE, LT_STORED_MOMENTUM};  // eval_momentum
    return {{cond_only ? LT_KIND_COND_ONLY : o.cfg_rule ? LT_KIND_RULE : LT_KIND_DEV_GUIDED, LT_KIND_COUNT}, 1, LT_SCALE_TABLE, LT_STORED_NONE};
}

static void check_form(const char* name, const GuidancePlan& plan, const Old& o, int ncalls_table) {
    for (int call = 0; call < ncalls_table; ++call) {
        const GuidanceStep got = plan.step_of(call), want = old_eval(o, call);
        if (got.n_kinds != want.n_kinds) fail(name, call, "the number of kinds", got.n_kinds, want.n_kinds);
        for (int k = 0; k < want.n_kinds && k < got.n_kinds; ++k)
            if (got.kinds[k] != want.kinds[k]) fail(name, call, k ? "the closing kind" : "the first kind", got.kinds[k], want.kinds[k]);
        if (got.scale != want.scale) fail(name, call, "the scale word", got.scale, want.scale);
        if (got.rewrites != want.rewrites) fail(name, call, "the stored buffer", got.rewrites, want.rewrites);
    }
    // the tail: ode_fixed_grid's count and copies (ode_multistep's are the same expression with stages = 1 and no slg / project)
    const bool cs = o.cfg_host != nullptr;
    for (int stages : {1, 2, 4})
        for (int B : {2, 4})
            for (int n_grid : {2, 3}) {
                const int ncalls = (n_grid - 1) * stages;
                if (ncalls > ncalls_table) continue;
                const int nsent = ncalls * B + (cs ? ncalls : 0) + (cs && o.rule ? 2 : 0) + (cs && o.slg_host ? ncalls : 0) + (cs && o.project ? 3 : 0);
                const int tail = plan.tail_floats(ncalls);
                if (ncalls * B + tail != nsent) fail(name, ncalls, "the floats sent", ncalls * B + tail, nsent);
                if (GuidancePlan::table_offset(ncalls, B) != (size_t)ncalls * B)
                    fail(name, ncalls, "the table's offset", (int)GuidancePlan::table_offset(ncalls, B), ncalls * B);
                if (GuidancePlan::second_offset(ncalls, B) != (size_t)ncalls * B + ncalls)
                    fail(name, ncalls, "the second block's offset", (int)GuidancePlan::second_offset(ncalls, B), ncalls * B + ncalls);
                // exactly `tail` floats written, each what the former memcpys put there, nothing beyond (the buffer ends where the tail ends:
                // the address sanitizer sees a write past it; the canary in front and the slack inside a second buffer see the rest)
                const float canary = -12345.25f;
                std::vector<float> exact((size_t)nsent, canary), roomy((size_t)nsent + 8, canary), want_buf((size_t)nsent + 8, canary);
                plan.fill_tail(exact.data() + GuidancePlan::table_offset(ncalls, B), ncalls);
                plan.fill_tail(roomy.data() + GuidancePlan::table_offset(ncalls, B), ncalls);
                float* tp = want_buf.data();
                if (cs) memcpy(tp + (size_t)ncalls * B, o.cfg_host, (size_t)ncalls * sizeof(float));
                if (cs && o.rule) memcpy(tp + (size_t)ncalls * B + ncalls, o.rule, 2 * sizeof(float));
                if (cs && o.slg_host) memcpy(tp + (size_t)ncalls * B + ncalls, o.slg_host, (size_t)ncalls * sizeof(float));
                if (cs && o.project) memcpy(tp + (size_t)ncalls * B + ncalls, o.project, 3 * sizeof(float));
                for (int i = 0; i < nsent + 8; ++i) {
                    if (memcmp(&roomy[i], &want_buf[i], sizeof(float)) != 0) fail(name, ncalls, "a word of the filled buffer differs, word", i, i);
                    if (i < nsent && memcmp(&exact[i], &want_buf[i], sizeof(float)) != 0) fail(name, ncalls, "a word of the exact buffer differs, word", i, i);
                }
                for (int i = 0; i < tail; ++i)  // (every table value below differs from the canary, so each of the `tail` floats was written)
                    if (roomy[(size_t)ncalls * B + i] == canary) fail(name, ncalls, "a tail word was left unwritten, word", i, i);
            }
}

int main() {
    // eight evaluations (a 3-point rk4 grid): a scale of exactly 1, the float next to 1, 0, a negative one; against the reuse flags 0 and 1 and
    // the skip-layer scales 0 and non-zero every combination occurs, among them "scale 1, reuse flag 1" and "scale 1, s != 0"
    const float near1 = std::nextafterf(1.0f, 2.0f);
    const float table[8] = {1.0f, near1, 0.0f, -2.5f, 1.0f, near1, 0.0f, -2.5f};
    const int32_t flags[8] = {0, 0, 0, 0, 1, 1, 1, 1};
    const float slg[8] = {0.0f, 0.0f, 0.0f, 0.0f, 3.0f, -1.5f, 0.25f, 2.0f};
    const float rule[2] = {0.7f, 12.0f}, par[3] = {0.5f, -0.75f, 15.0f};
    const int32_t skip[2] = {1, 3}, perturb[1] = {2};
    CacheControl cc;

    Old o;
    check_form("none", GuidancePlan{}, o, 8);
    o = Old{}; o.cfg_host = table;
    check_form("table", GuidancePlan::of_table(table), o, 8);
    o = Old{}; o.cfg_host = table; o.cfg_rule = true; o.rule = rule;
    check_form("rule", GuidancePlan::of_rule(table, rule), o, 8);
    o = Old{}; o.cfg_host = table; o.reuse_host = flags;
    check_form("reuse", GuidancePlan::of_reuse(table, flags), o, 8);
    o = Old{}; o.cfg_host = table; o.slg_host = slg;
    check_form("slg", GuidancePlan::of_slg(table, slg, skip, 2, nullptr, 0, false), o, 8);
    check_form("pag", GuidancePlan::of_slg(table, slg, skip, 2, perturb, 1, true), o, 8);
    o = Old{}; o.cfg_host = table; o.cfg_rule = true; o.rule_form = 1; o.project = par;
    check_form("project apg", GuidancePlan::of_project(table, true, 1, par[0], par[1], par[2], 0), o, 8);
    o.rule_form = 2;
    check_form("project zero-star", GuidancePlan::of_project(table, false, 2, par[0], par[1], par[2], 1), o, 8);
    o = Old{}; o.cache = true;
    check_form("cached", GuidancePlan::of_cache(&cc), o, 8);

    // the reuse and slg tables again with the flag / scale columns swapped, so that every scale meets both values in both halves
    const int32_t flags2[8] = {1, 1, 1, 1, 0, 0, 0, 0};
    const float slg2[8] = {3.0f, -1.5f, 0.25f, 2.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    o = Old{}; o.cfg_host = table; o.reuse_host = flags2;
    check_form("reuse, flags swapped", GuidancePlan::of_reuse(table, flags2), o, 8);
    o = Old{}; o.cfg_host = table; o.slg_host = slg2;
    check_form("slg, scales swapped", GuidancePlan::of_slg(table, slg2, skip, 2, nullptr, 0, false), o, 8);

    // the combinations by name
    if (GuidancePlan::of_reuse(table, flags).step_of(4).kinds[0] != LT_KIND_COND_ONLY) fail("reuse", 4, "scale 1 under flag 1", 0, LT_KIND_COND_ONLY);
    if (GuidancePlan::of_reuse(table, flags).step_of(5).kinds[0] != LT_KIND_REUSE_AGAIN) fail("reuse", 5, "the scale next to 1 under flag 1", 0, LT_KIND_REUSE_AGAIN);
    if (GuidancePlan::of_slg(table, slg, skip, 2, nullptr, 0, false).step_of(4).kinds[1] != LT_KIND_SLG_COND) fail("slg", 4, "scale 1 at s != 0", 0, LT_KIND_SLG_COND);
    if (GuidancePlan::of_slg(table, slg, skip, 2, nullptr, 0, false).step_of(0).kinds[0] != LT_KIND_COND_ONLY) fail("slg", 0, "scale 1 at s = 0", 0, LT_KIND_COND_ONLY);
    if (failures) { std::printf("guidance_plan: %d failure(s)\n", failures); return 1; }
    std::printf("guidance_plan: ok\n");
    return 0;
}
