// The kinds of one model evaluation (forward_graphed, engine.h) and what the engine derives from a kind.  Includes nothing, so that
// tests/host/eval_kind.hip compiles it alone.
#pragma once

enum LtEvalKind {
    LT_KIND_WHOLE = 0,     // guidance scale from the host (a->cfg_scale; use_cfg 0 or 1) - the only kind a packed batch takes
    LT_KIND_DEV_GUIDED,    // scale from device memory, all rows guided
    LT_KIND_COND_ONLY,     // ... a scale of 1: the first a->batch / 2 rows on the first half of the conditioning, written to both halves of `out`
    LT_KIND_RULE,          // guided, times the per-sample factor of the rescale / norm-limit rule whose parameters are in e->g_cfg[1..2]
    LT_KIND_REUSE_STORE,   // guided, the cond - uncond difference of the guided channels also stored in e->g_delta
    LT_KIND_REUSE_AGAIN,   // the cond rows, guided with the stored difference, both halves written
    LT_KIND_SLG_STORE,     // skip-layer / perturbed-attention guidance: the cond rows under the caller's SkipScope (blocks left out and / or perturbed), guided channels to e->g_skip, `out` unused
    LT_KIND_SLG_GUIDED,    // ... all rows, the closing kernel adds s (cond - skip) with s from e->g_cfg[3]
    LT_KIND_SLG_COND,      // ... the cond rows alone, cond + s (cond - skip), both halves written
    LT_KIND_CACHE_HEAD,    // step caching: patchify .. the first pre-norm + modulate, the indicator sums (e->c_ws), x_0 kept; `out` unused
    LT_KIND_CACHE_BLOCKS,  // ... the L blocks, r = bfr(x_L - x_0) stored, the tail: `out` is the whole evaluation's word for word; follows its head
    LT_KIND_CACHE_APPLY,   // ... x = bfr(x_0 + r), the final layer's norm + modulate, the tail - no block launches anything; follows its head
    LT_KIND_COUNT
};

struct LtEvalTraits {
    bool dev_scale;   // the guidance scale is read from device memory (e->g_cfg); the host's a->cfg_scale is ignored
    bool half;        // evaluates a->batch / 2 rows, on the first half of the prepared conditioning; its output has a->batch rows
    bool reads_x;     // reads the state x_in (and runs patchify .. the first pre-norm)
    bool writes_out;  // writes `out`
    bool rule;        // the rule's parameters e->g_cfg[1..2] are used
    bool skip_ok;     // may run under a layer-skip set and / or a perturbed-attention set (SkipScope)
    bool cached;      // a part of an evaluation under step caching: hands e->x / e->h / e->mod to the next part
};

constexpr LtEvalTraits lt_eval_traits(LtEvalKind k) {
    switch (k) {  //                     dev    half   reads  writes rule   skip   cached
    case LT_KIND_WHOLE:        return {false, false, true,  true,  false, true,  false};  // (a set: lt_forward_skip / lt_forward_perturb)
    case LT_KIND_DEV_GUIDED:   return {true,  false, true,  true,  false, false, false};
    case LT_KIND_COND_ONLY:    return {true,  true,  true,  true,  false, false, false};
    case LT_KIND_RULE:         return {true,  false, true,  true,  true,  false, false};
    case LT_KIND_REUSE_STORE:  return {true,  false, true,  true,  false, false, false};
    case LT_KIND_REUSE_AGAIN:  return {true,  true,  true,  true,  false, false, false};
    case LT_KIND_SLG_STORE:    return {true,  true,  true,  false, false, true,  false};
    case LT_KIND_SLG_GUIDED:   return {true,  false, true,  true,  false, false, false};
    case LT_KIND_SLG_COND:     return {true,  true,  true,  true,  false, false, false};
    case LT_KIND_CACHE_HEAD:   return {false, false, true,  false, false, false, true};
    case LT_KIND_CACHE_BLOCKS: return {false, false, false, true,  false, false, true};
    case LT_KIND_CACHE_APPLY:  return {false, false, false, true,  false, false, true};
    case LT_KIND_COUNT:        break;
    }
    return {};
}

// the mode argument of unpatchify_cfg_slg_kernel (guidance_skip.hip) for the three skip-layer kinds; -1 for every other kind
constexpr int lt_slg_kernel_mode(LtEvalKind k) {
    return k == LT_KIND_SLG_STORE ? 0 : k == LT_KIND_SLG_GUIDED ? 1 : k == LT_KIND_SLG_COND ? 2 : -1;
}
