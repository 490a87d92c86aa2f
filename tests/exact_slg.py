"""Skip-layer guidance restated independently of torch's bf16 arithmetic, and the model surgery of its exact layer-skip oracles.

The chain: float64 numpy with explicit roundings, ``R`` = ``exact_reuse.bf16_round64`` (the exact float64 result of one fp32 operation on bf16 /
fp32 operands, rounded to fp32 and then to bf16).  Five roundings with guidance, three at ``w == 1``.

The surgery: ``zero_gates`` makes blocks the identity by zeroing the rows of their ``adaLN_modulation`` that produce their gates (a block then
adds ``0 * y`` to the residual stream); ``drop_layers`` removes blocks from a state dict and renumbers the rest."""
import re

import numpy as np
import torch

from exact_reuse import bf16_round64, prod_bf16

# the gate chunks of a block's adaLN_modulation output (of `chunks` equal parts), per family (oracle.synth.NextDiTConfig.family)
GATE_CHUNKS = {"next_t2i": (4, (1, 3)), "imagenet": (4, (1, 3)), "moe_time": (4, (1, 3)), "moe_space": (4, (1, 3)), "moe": (6, (1, 3, 5)),
               "flag_t2i": (6, (2, 5))}


def slg_chain(c, u, k, w, s):
    """R(R(u + R(w R(c - u))) + R(s R(c - k))); u None (the stage at w == 1): R(c + R(s R(c - k))).  float64 arrays of bf16 values"""
    t = prod_bf16(s, bf16_round64(c - k))
    if u is None:
        return bf16_round64(c + t)
    return bf16_round64(bf16_round64(u + prod_bf16(w, bf16_round64(c - u))) + t)


def tie_operands(w, s):
    """(c, u, k) bf16 tensors [128] on which w d, s (c - k) and both sums meet bf16 ties.

    d = c - u = 1 + i / 128 and e = c - k = 1 + ((5 i) % 128) / 128 (i = 0..124) use all 8 significand bits, so their products with 1.5, 2.5,
    4.5 carry 9 or 10 significant bits, half of them exactly between two bf16 values.  u = (i % 3) / 128 is a multiple of 2^-7 next to
    R(w d) in [1.5, 9), whose ulp is 2^-7 .. 2^-4: the first sum has bits below the ulp, ties among them; the second adds two such values
    of different binades.  c = u + d < 2 and k = c - e (|k| < 1) are multiples of 2^-7, so bf16 values, and both differences are exact."""
    i = torch.arange(125, dtype=torch.float32)
    d = 1.0 + i / 128.0
    e = 1.0 + ((5 * i) % 128) / 128.0
    u = (i % 3) / 128.0
    c = u + d
    k = c - e
    out = [t.to(torch.bfloat16) for t in (c, u, k)]
    for got, want in zip(out, (c, u, k)):
        assert torch.equal(got.float(), want)  # bf16 values, as claimed
    assert torch.equal((out[0] - out[1]).float(), d) and torch.equal((out[0] - out[2]).float(), e)
    return out


def count_ties(x):
    """how many of the exact float64 values lie exactly between two neighbouring bf16 values"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    m, ex = np.frexp(x)  # x = m 2^ex, m in [0.5, 1): the bf16 grid of the binade has steps of 2^(ex - 8)
    q = m * 512.0  # in units of half a step
    return int(np.sum((q == np.floor(q)) & (np.floor(q) % 2 == 1)))


def zero_gates(sd, family, layers, dim):
    """a copy of the state dict in which the blocks `layers` are the identity: the gate rows of their adaLN_modulation, weight and bias, zeroed"""
    chunks, gates = GATE_CHUNKS[family]
    out = {k: v.clone() for k, v in sd.items()}
    for l in layers:
        for suffix in ("weight", "bias"):
            t = out[f"layers.{l}.adaLN_modulation.1.{suffix}"]
            assert t.shape[0] == chunks * dim, (t.shape, chunks, dim)
            for g in gates:
                t[g * dim:(g + 1) * dim] = 0
    return out


def drop_layers(sd, layers):
    """the state dict of the model without the blocks `layers`, the others renumbered in order"""
    keep = sorted({int(m.group(1)) for k in sd for m in [re.match(r"layers\.(\d+)\.", k)] if m} - set(layers))
    new = {old: i for i, old in enumerate(keep)}
    out = {}
    for k, v in sd.items():
        m = re.match(r"layers\.(\d+)\.(.*)", k)
        if not m:
            out[k] = v
        elif int(m.group(1)) in new:
            out[f"layers.{new[int(m.group(1))]}.{m.group(2)}"] = v
    return out
