"""CPU: the draws of tests/test_gpu_attention_nk.py (tests/attention_nk_cases.py) satisfy what the word-exact comparison rests on, so the
GPU test cannot hide behind its own allowance: expected() accepts every draw, the share of words with two admissible values stays under
MAX_AMBIGUOUS, the reduction indices are exercised by VALID keys alone, and expected() still refuses a draw whose off keys could decide
a word.  The poisoned rows never reach the expectation."""
import pytest
import torch

import attention_nk_cases as K
import exact_attention as X


@pytest.fixture(scope="module")
def self_draws():
    """(family, case) -> (draw, float64 expectation), computed once"""
    out = {}
    for fam in K.FAMILIES:
        for case in K.SELF_CASES:
            inp = K.draw(fam, *case)
            out[fam, case] = (inp, X.expected(inp))  # a PreconditionError here fails every test below: the draw is not usable
    return out


def test_expected_accepts_every_draw_and_few_words_are_ambiguous(self_draws):
    for (fam, case), (inp, want) in self_draws.items():
        _, _, amb = X.admissible([want], lambda o: o)
        share = float(amb.double().mean())
        print(f"NK-DRAW {fam} {case} ambiguous {share:.4%} stats {inp['stats']}")
        assert share <= X.MAX_AMBIGUOUS, (fam, case, share)
        if fam == "selector":
            assert inp["stats"]["max_live"] == 1
        elif max(case[4]) > 64:
            assert inp["stats"]["jump"] > 0 and inp["stats"]["small_raise"] > 0, (case, inp["stats"])  # the deferred maximum moves both ways


def test_fused_draws_are_accepted_on_both_sides():
    for fam in K.FAMILIES:
        for B, H, Hkv, N, counts, T, tvalid in K.FUSED_CASES:
            a, t = K.fused_draw(fam, B, H, Hkv, N, counts, T, tvalid)
            ws, wt = X.expected(a), X.expected(t)
            _, _, amb = X.admissible([ws, wt], X.fused(X.gate_values(H, T)))
            assert float(amb.double().mean()) <= X.MAX_AMBIGUOUS, (fam, counts, T)
            # masking the image keys takes no reduction index away that the full-length draw exercises
            full = dict(a, valid=[N] * B)
            assert K.restricted_use(a)[0] == K.restricted_use(full)[0] and a["valid"] == list(counts)


def test_every_reduction_index_is_used_by_valid_keys_alone(self_draws):
    """levels: in every sample with at least two valid keys each of the 72 reduction indices multiplies a non-zero q by a non-zero k of a
    VALID key in every whole 64-row block of every head; a single-key sample cannot (its key has zeros: the class dims are one-hot) -
    there every index on which the one valid key is non-zero must meet a non-zero q"""
    for (fam, case), (inp, _) in self_draws.items():
        if fam != "levels":
            continue
        B, H, Hkv, N, counts = case
        shares = K.restricted_use(inp)
        for b, n in enumerate(counts):
            if n >= 2:
                assert shares[b] == 1.0, (case, b, shares)
            else:
                rep = H // Hkv
                kn = (inp["k"][b, :, :n] != 0).any(1).repeat_interleave(rep, 0)
                qn = (inp["q"][b, :, :N // 64 * 64] != 0).view(H, N // 64, 64, K.HD).any(2)
                assert bool((qn | ~kn[:, None, :]).all()), (case, b)
        assert X.every_reduction_index_is_used(inp) == all(n >= 2 for n in counts)


def test_poison_touches_masked_rows_only_and_stays_finite(self_draws):
    for (fam, case), (inp, _) in self_draws.items():
        k, v = K.poison_masked(inp)
        Nk = k.shape[2]
        for b, n in enumerate(inp["valid"]):
            assert torch.equal(k[b, :, :n], inp["k"][b, :, :n]) and torch.equal(v[b, :, :n], inp["v"][b, :, :n])
            if n < Nk:
                for t in (k, v):
                    m = t[b, :, n:].float()
                    assert bool(torch.isfinite(m).all()) and float(m.abs().min()) >= 1024 and float(m.abs().max()) <= 1536
                    assert bool((m > 0).any()) and bool((m < 0).any())
        # |q . k| with a poisoned key stays far inside fp32: no score overflows
        assert K.HD * float(inp["q"].float().abs().max()) * 1536 < 2 ** 24


def test_expected_refuses_a_draw_whose_off_keys_could_decide_a_word():
    B, H, Hkv, N, counts = 3, 2, 2, 320, (320, 191, 64)
    inp = K.draw("levels", B, H, Hkv, N, counts)
    b, h, row = 1, 0, 5
    s = inp["q"][b, h, row].double() @ inp["k"][b, h].double().t()
    s[counts[b]:] = float("-inf")
    rel = s - s.max()
    live, off = rel >= -(X.NLEVEL - 1), (rel <= -64) & torch.isfinite(rel)
    assert int(live.sum()) >= 1 and int(off.sum()) >= 1
    inp["v"][b, h, live, 0] = 0  # the live keys of word (row, 0) add nothing: the off keys would decide it
    with pytest.raises(X.PreconditionError, match="off keys would decide"):
        X.expected(inp)


def test_case_lists_cover_the_mechanisms():
    tiles = lambda n: (n + 63) // 64  # noqa: E731
    flat = [(N, n) for _, _, _, N, c in K.SELF_CASES for n in c]
    assert any(tiles(n) > 4 and n % 64 for N, n in flat)            # mask written inside the tile loop (the ring slot is reused)
    assert any(tiles(n) <= 4 and n % 64 for N, n in flat)           # mask written with the constants
    assert any(n % 64 == 0 and n < N for N, n in flat)              # fewer whole tiles, no mask
    assert any(n == 1 for _, n in flat) and any(n % 64 == 1 and n > 64 for _, n in flat) and any(n % 64 == 63 for _, n in flat)
    assert {(B * H) % 8 == 0 for B, H, _, _, _ in K.SELF_CASES} == {True, False} and any(H != Hkv for _, H, Hkv, _, _ in K.SELF_CASES)
    assert all(N % 64 == 0 and N % 256 for _, _, _, N, _ in K.SELF_CASES)  # whole key tiles, a partial query block
