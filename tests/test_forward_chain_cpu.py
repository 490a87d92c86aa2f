"""The operator chain of tests/forward_chain.py IS the model (no GPU): its float64 backend against the fp32 oracle, and every wiring mutation
of the list against the gate.

Gate.  `Torch64` has no rounding inside, the oracle (oracle/nextdit_oracle.py, oracle/variants_oracle.py, fp32, on the same bf16-valued
weights and inputs) has fp32's: rel_l2(torch64, oracle) measures the oracle's own rounding.  MEASURED below holds the value of every case
(profiles/forward_chain/CPU_DISTANCES.md is the same table); GATE is 4 times the largest.  A chain that states one argument differently from
the reference moves the output by far more: the second test runs every mutation of forward_chain.mutations through the float64 backend and
requires each to move the output by MORE than the gate - which shows both that the gate can see the argument and that the output of the
fixture depends on it (the condition under which bit equality on the GPU, tests/test_gpu_forward_chain.py, proves anything about it).

Mixture-of-experts cases.  Routing is discrete, so before any output is compared the chain's selections must equal the ones the fp32 oracle
records (variants_oracle.MoeRouting) for EVERY row of every layer and branch; a mismatch names the row and the margin between its second
and third logit.  On the fixtures used here float64 and fp32 agree on every row (smallest margin 4e-3 against fp32's 1e-6), so the distance
measured is the oracle's rounding alone, as for the dense families."""
import pytest

import numpy as np

import forward_chain as FC

# rel_l2(torch64, fp32 oracle), measured; the test prints the value of the run beside it
MEASURED = {
    "nextdit_tiny-forward": 9.871e-07, "nextdit_tiny-cfg4": 1.152e-06, "nextdit_tiny-lin2": 1.158e-06, "nextdit_tiny-ntk2": 1.079e-06,
    "nextdit_tiny_rect-forward": 1.005e-06, "nextdit_tiny_rect-cfg4": 1.295e-06, "nextdit_tiny_rect-lin2": 1.229e-06,
    "nextdit_tiny_rect-ntk2": 1.216e-06, "nextdit_tiny_gqa-forward": 9.629e-07, "nextdit_tiny_gqa-cfg4": 1.180e-06,
    "nextdit_tiny_gqa-lin2": 1.080e-06, "nextdit_tiny_gqa-ntk2": 1.111e-06, "imagenet_tiny-forward": 6.833e-07, "imagenet_tiny-cfg4": 2.362e-06,
    "flag_tiny-forward": 8.041e-07, "flag_tiny-cfg4": 8.164e-07,
    "moe_time_tiny-forward": 7.748e-07, "moe_time_tiny-cfg4": 2.447e-06, "moe_time_tiny-cfg4-t2": 1.843e-06, "moe_time_tiny-eps": 2.040e-06,
    "moe_space_tiny-forward": 9.345e-07, "moe_space_tiny-cfg4": 2.882e-06, "moe_space_tiny-cfg4-t2": 3.264e-06, "moe_space_tiny-eps": 2.219e-06,
    "moe_tiny-forward": 1.064e-06, "moe_tiny-cfg4": 2.821e-06, "moe_tiny-cfg4-t2": 2.948e-06, "moe_tiny-eps": 2.376e-06,
}
GATE = 4 * max(MEASURED.values())     # 1.31e-5 (moe_space_tiny-cfg4-t2; 9.45e-6 before the mixture-of-experts cases)

MODEL_CASES = [(name, mode) for fam, names in FC.GOLDENS.items() for name in names
               for mode in ("forward", "cfg4") + (("lin2", "ntk2") if fam == "next_t2i" else ())] + \
              [(name, mode) for name in FC.MOE_GOLDENS for mode in ("cfg4-t2", "eps")]
# the cases the mutations run on: guidance 4 on every fixture, both RoPE branches where the family has them, the batch of three images, and
# the small-row cases of the eps entries
MUTATION_CASES = [(name, "cfg4") for names in FC.GOLDENS.values() for name in names] + \
                 [(name, mode) for name in FC.GOLDENS["next_t2i"] for mode in ("lin2", "ntk2")] + \
                 [("nextdit_tiny", "batch6"), ("nextdit_tiny", "eps"), ("imagenet_tiny", "eps"), ("imagenet_tiny", "eps-unfused"), ("flag_tiny", "eps")] + \
                 [(name, mode) for name in FC.MOE_GOLDENS for mode in ("cfg4-t2", "eps")] + [("moe_tiny", "cfg4-t2-unrouted")]
# (cfg4-t2: the two samples at different timesteps, so that their time routers differ; cfg4-t2-unrouted: family moe with the space router as a
# step of its own, paths route_fused False - the form in which the router's input is an argument)


def make_case(golden_dir, name, mode):
    """-> (case, paths)"""
    if mode == "batch6":
        return FC.batch6_case(golden_dir), {}
    if mode.startswith("eps"):
        return FC.eps_case(golden_dir, name), {"small_fused": mode == "eps"}
    if mode.endswith("-unrouted"):
        return FC.golden_case(golden_dir, name, mode[:-len("-unrouted")]), {"route_fused": False}
    return FC.golden_case(golden_dir, name, mode), {}


def run_against_oracle(case, steps):
    """-> (the float64 chain's output, rel_l2 to the fp32 oracle); a mixture-of-experts case first has every row's selection compared"""
    from oracle import variants_oracle as V
    be = FC.Torch64(case)
    got = FC.run(be, steps)
    hook = V.MoeRouting(case.cfg.n_layers) if case.fam.get("moe") else None
    want = FC.oracle_fp32(case, hook) if hook else FC.oracle_fp32(case)
    if hook:
        branches = {0: "time", 1: "space"}
        assert sorted(hook.rec) == sorted((l, b) for l in range(case.cfg.n_layers) for b in branches if any(br == branches[b] for br, _ in case.fam["moe"]))
        assert len(be.sel) == len(hook.rec)
        for (l, b), rec in hook.rec.items():
            key = f"sel.l{l}.{branches[b]}"
            mine = be.sel[key].numpy()
            assert mine.shape == rec.shape == (case.B * case.N, 2), (case.name, key, mine.shape, rec.shape)
            bad = np.nonzero((mine != rec).any(1))[0]
            if bad.size:
                top = be.logits[key][int(bad[0])].topk(3).values
                raise AssertionError(f"{case.name} {key}: {bad.size} rows select differently, first row {int(bad[0])}: chain {mine[bad[0]].tolist()}, oracle "
                                     f"{rec[bad[0]].tolist()}, margin between its second and third logit {float(top[1] - top[2]):.3e}")
    return got, FC.rel_l2(got, want)


@pytest.mark.parametrize("name,mode", MODEL_CASES)
def test_float64_chain_is_the_oracle(golden_dir, name, mode):
    case, paths = make_case(golden_dir, name, mode)
    _, err = run_against_oracle(case, FC.build(case, paths))
    print(f"{case.name}: rel_l2(torch64, oracle fp32) = {err:.3e} (recorded {MEASURED[case.name]:.3e}, gate {GATE:.3e})")
    assert err < GATE, (case.name, err, GATE)


@pytest.mark.parametrize("name,mode", MUTATION_CASES)
def test_every_mutation_moves_the_float64_chain_past_the_gate(golden_dir, name, mode):
    case, paths = make_case(golden_dir, name, mode)
    steps = FC.build(case, paths)
    base, err = run_against_oracle(case, steps)
    assert err < GATE, (case.name, "unmutated", err)     # (also the cases that are no fixture call: the batch of three, the small rows)
    muts = FC.mutations(case, steps)
    assert muts, case.name
    missed = []
    for mname, hook in muts:
        moved = FC.rel_l2(FC.run(FC.Torch64(case), steps, hook), base)
        print(f"{case.name}: {mname}: moved {moved:.3e}")
        if not moved > GATE:
            missed.append((mname, moved))
    assert not missed, (case.name, GATE, missed)


# ---- the large-row regime's step list, at the tiny fixtures' shapes ---------------------------------------------------------------------------
# Which launch runs is a property of the GPU launchers (from one 256-row tile per CU on); what the steps MEAN is not, so the float64 backend
# runs every large-regime list on the fixtures and is held to the oracle by the same gate (tests/test_gpu_forward_chain_large.py runs the same
# lists on the GPU at the sizes where the engine takes these routes).
LARGE_PATHS = {
    "qraw": {"qkv": "fused", "raw_q": True, "ystat": 1},                    # QKV_FUSED + raw_q / POST_K_ONLY: next_t2i at head_dim 72
    "pair": {"qkv": "fused", "post": "pair", "ystat": 1},                   # QKV_FUSED + POST_QK_PAIR: head_dim 48 / 96 / 128, or attn_q_fused 0
    "qk_vt": {"qkv": "qk_vt", "post": "pair", "ystat": 1},                  # qkv_fused_gemm 0: Q | K plain + the V^T launch
    "pair_reduce": {"qkv": "fused", "post": "pair", "ystat": 0},            # grn_ystat 0: the closing steps reduce y themselves
    "qraw_reduce": {"qkv": "fused", "raw_q": True, "ystat": 0},
}
LARGE_CASES = [(name, mode, key) for name in FC.GOLDENS["next_t2i"] for mode in ("cfg4", "lin2", "ntk2") for key in ("qraw", "pair")] + \
              [("nextdit_tiny_gqa", "forward", "qraw"), ("nextdit_tiny_rect", "cfg4", "qk_vt"), ("nextdit_tiny", "cfg4", "pair_reduce"),
               ("nextdit_tiny_gqa", "cfg4", "qraw_reduce")] + \
              [(name, mode, key) for name in ("imagenet_tiny", "flag_tiny") for mode in ("forward", "cfg4") for key in ("pair", "qk_vt")]
LARGE_MUTATION_CASES = [("nextdit_tiny_rect", "lin2", "qraw"), ("nextdit_tiny_gqa", "ntk2", "qraw"), ("nextdit_tiny_rect", "ntk2", "pair"),
                        ("nextdit_tiny_rect", "cfg4", "qk_vt"), ("imagenet_tiny", "cfg4", "pair"),
                        ("flag_tiny", "cfg4", "qk_vt")]


@pytest.mark.parametrize("name,mode,key", LARGE_CASES)
def test_large_regime_step_list_is_the_oracle(golden_dir, name, mode, key):
    case, _ = make_case(golden_dir, name, mode)
    steps = FC.build(case, LARGE_PATHS[key])
    default = {s.name for s in FC.build(case, {"small_fused": False})}
    assert {s.name for s in steps} != default, "the paths changed no step"
    _, err = run_against_oracle(case, steps)
    print(f"{case.name} [{key}]: rel_l2(torch64, oracle fp32) = {err:.3e} (default list: {MEASURED[case.name]:.3e}, gate {GATE:.3e})")
    assert err < GATE, (case.name, key, err, GATE)


@pytest.mark.parametrize("name,mode,key", LARGE_MUTATION_CASES)
def test_large_regime_mutations_move_the_float64_chain_past_the_gate(golden_dir, name, mode, key):
    """every mutation of the new steps that float64 models ("gpu:" entries change operands it does not: the GPU module runs those)"""
    case, _ = make_case(golden_dir, name, mode)
    steps = FC.build(case, LARGE_PATHS[key])
    base, err = run_against_oracle(case, steps)
    assert err < GATE, (case.name, key, "unmutated", err)
    muts = [(m, h) for m, h in FC.large_mutations(case, steps) if not m.startswith("gpu:")]
    assert muts, (case.name, key)
    missed = []
    for mname, hook in muts:
        moved = FC.rel_l2(FC.run(FC.Torch64(case), steps, hook), base)
        print(f"{case.name} [{key}]: {mname}: moved {moved:.3e}")
        if not moved > GATE:
            missed.append((mname, moved))
    assert not missed, (case.name, key, GATE, missed)


def test_mutation_list_covers_the_issue(golden_dir):
    """every entry of the list appears on at least one case, in layer 0 and layer 1 where it is per layer"""
    seen = set()
    for name, mode in MUTATION_CASES:
        case, paths = make_case(golden_dir, name, mode)
        seen |= {m for m, _ in FC.mutations(case, FC.build(case, paths))}
    per_layer = ["pre_norms_swapped", "post_norms_swapped", "q_k_norm_weight_swapped", "q_norm_bias_dropped", "qk_ln_eps_1e-6", "ky_ln_eps_1e-6",
                 "self_scale_without_proportional", "text_scale_with_proportional", "text_gate_heads_exchanged", "rope_branch_flipped"]
    once = ["l1.reads_layer0_pre_norm", "l1.reads_layer0_post_norm", "l1.chunk_from_layer0:l0.grn_ffn.next_scale",
            "l1.chunk_from_layer0:l0.grn_ffn.next_shift", "l1.chunk_from_layer0:l1.grn_attn.gate", "l1.chunk_from_layer0:l1.grn_attn.next_scale",
            "l1.chunk_from_layer0:l1.grn_attn.next_shift", "l1.chunk_from_layer0:l1.grn_ffn.gate", "final_adaln_bias_dropped",
            "cap_embedder_ln_bias_dropped", "norm_eps_1e-6", "norm_eps_1e-6@prep.l0.ynorm", "norm_eps_1e-6@prep.l1.ynorm", "norm_eps_1e-6@l0.prenorm",
            "norm_eps_1e-6@l0.grn_attn", "norm_eps_1e-6@l0.grn_ffn", "norm_eps_1e-6@l1.grn_attn", "norm_eps_1e-6@l1.grn_ffn", "final_ln_eps_1e-5",
            "final_shift_scale_exchanged", "gate_without_tanh:attn", "gate_without_tanh:ffn", "one_plus_scale_as_scale:attn",
            "one_plus_scale_as_scale:ffn", "one_plus_scale_as_scale:final", "text_bias_from_other_row", "rope_row_col_exchanged", "cfg_channels_3_4", "cfg_pairing_shifted",
            "eol_token_omitted", "x_embedder_bias_dropped"]
    # the mixture-of-experts wirings: per layer, per layer and branch, and the "layer 1 reads layer 0's" forms
    per_layer += ["time_space_expert_weights_exchanged", "time_space_router_weights_exchanged", "ffn_norms_time_space_exchanged",
                  "ffn_branch_chunks_exchanged", "space_combined_through_time_plan", "fused_router_in_attention_closing_step",
                  "time.experts_exchanged_in_w13_not_w2", "space.experts_exchanged_in_w13_not_w2", "time.w1_w3_exchanged_in_packing",
                  "space.w1_w3_exchanged_in_packing", "time.combine_weights_exchanged", "space.combine_weights_exchanged", "time.rows_per_sample_halved",
                  "space.router_fed_residual_stream"]
    once += ["l1.time.logits_at_layer0_columns", "l1.time.router_weight_from_layer0", "l1.space.router_weight_from_layer0",
             "l1.time.expert_stack_from_layer0", "l1.space.expert_stack_from_layer0", "time_router_fed_adaln_in"]
    want = {f"l{l}.{m}" for m in per_layer for l in (0, 1)} | set(once)
    assert want <= seen, sorted(want - seen)
