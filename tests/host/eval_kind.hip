// Host only: the traits of the kinds of a model evaluation (csrc/eval_kind.h) against the rules the engine applied before the kinds had one
// name each, written out here literally - the sets below are the conditions of the former code, not a copy of the table.  Its own main; links
// nothing of the engine.
#include <cstdio>
#include <initializer_list>

#include "eval_kind.h"

static int failures = 0;

static bool in(LtEvalKind k, std::initializer_list<LtEvalKind> set) {
    for (LtEvalKind m : set) if (m == k) return true;
    return false;
}

static void expect(bool got, bool want, const char* what, int k) {
    if (got != want) { std::printf("kind %d: %s is %d, the rule says %d\n", k, what, (int)got, (int)want); ++failures; }
}

// the table is usable where a constant is needed
static_assert(lt_eval_traits(LT_KIND_COND_ONLY).half && !lt_eval_traits(LT_KIND_WHOLE).dev_scale, "lt_eval_traits is constexpr");
static_assert(lt_slg_kernel_mode(LT_KIND_SLG_COND) == 2, "lt_slg_kernel_mode is constexpr");
static_assert(LT_KIND_WHOLE == 0 && LT_KIND_COUNT == 12, "twelve kinds, the whole evaluation first (a default-constructed EvalSpec)");

int main() {
    for (int i = 0; i < LT_KIND_COUNT; ++i) {
        const LtEvalKind k = (LtEvalKind)i;
        const LtEvalTraits t = lt_eval_traits(k);
        // the scale came from device memory whenever cfg_dev was passed: every guidance-schedule, rule, reuse and skip-layer evaluation
        expect(t.dev_scale, in(k, {LT_KIND_DEV_GUIDED, LT_KIND_COND_ONLY, LT_KIND_RULE, LT_KIND_REUSE_STORE, LT_KIND_REUSE_AGAIN, LT_KIND_SLG_STORE,
                                   LT_KIND_SLG_GUIDED, LT_KIND_SLG_COND}), "dev_scale", i);
        // half(): dup || reuse == REUSE || reuse == SLG_STORE || reuse == SLG_COND
        expect(t.half, in(k, {LT_KIND_COND_ONLY, LT_KIND_REUSE_AGAIN, LT_KIND_SLG_STORE, LT_KIND_SLG_COND}), "half", i);
        // the replay staged the state for segment == WHOLE || segment == HEAD
        expect(t.reads_x, !in(k, {LT_KIND_CACHE_BLOCKS, LT_KIND_CACHE_APPLY}), "reads_x", i);
        expect(t.reads_x, in(k, {LT_KIND_WHOLE, LT_KIND_DEV_GUIDED, LT_KIND_COND_ONLY, LT_KIND_RULE, LT_KIND_REUSE_STORE, LT_KIND_REUSE_AGAIN,
                                 LT_KIND_SLG_STORE, LT_KIND_SLG_GUIDED, LT_KIND_SLG_COND, LT_KIND_CACHE_HEAD}), "reads_x (listed)", i);
        // ... and copied `out` back for reuse != SLG_STORE && segment != HEAD
        expect(t.writes_out, !in(k, {LT_KIND_SLG_STORE, LT_KIND_CACHE_HEAD}), "writes_out", i);
        // the rule's parameters: rule && !cond_only
        expect(t.rule, k == LT_KIND_RULE, "rule", i);
        // a layer-skip set: of the kinds that read the scale from device memory the skip evaluation alone took one, a part of a step-cached
        // evaluation none; the whole evaluation takes one (lt_forward_skip)
        expect(t.skip_ok, in(k, {LT_KIND_SLG_STORE, LT_KIND_WHOLE}), "skip_ok", i);
        expect(t.cached, in(k, {LT_KIND_CACHE_HEAD, LT_KIND_CACHE_BLOCKS, LT_KIND_CACHE_APPLY}), "cached", i);
        // what never met: a part of a step-cached evaluation read no scale from device memory; a half-row kind read it there
        if (t.cached) expect(t.dev_scale, false, "dev_scale of a step-caching part", i);
        if (t.half) expect(t.dev_scale, true, "dev_scale of a half-row kind", i);
        // the kernel mode was reuse - LT_EVAL_SLG_STORE: store, guided, cond = 0, 1, 2
        const int mode = k == LT_KIND_SLG_STORE ? 0 : k == LT_KIND_SLG_GUIDED ? 1 : k == LT_KIND_SLG_COND ? 2 : -1;
        if (lt_slg_kernel_mode(k) != mode) { std::printf("kind %d: kernel mode %d, the rule says %d\n", i, lt_slg_kernel_mode(k), mode); ++failures; }
    }
    if (failures) { std::printf("eval_kind: %d failure(s)\n", failures); return 1; }
    std::printf("eval_kind: ok\n");
    return 0;
}
