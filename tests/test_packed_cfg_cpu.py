"""CPU: guidance on a size list.  The fixture tests/golden/nextdit_tiny_packed_cfg.npz (the unmodified reference's list forward + the guidance
expression, scripts/make_packed_cfg_golden.py) against the oracle's forward_packed plus the same expression; the host-side table of a packed
batch (offsets, counts, widths) against a plain Python restatement; the null-argument refusals of the new ABI calls.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from oracle import nextdit_oracle as O
from oracle import synth

PACKED_TOL = 2e-5  # tests/test_oracle_golden.py: the oracle's packed forward against the reference's list path


def test_oracle_forward_packed_plus_guidance_reproduces_the_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "nextdit_tiny_packed_cfg.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    sizes = [tuple(int(v) for v in hw) for hw in g["sizes"]]
    half = len(sizes)
    assert sizes == [(12, 20), (16, 16), (6, 16)] and cfg.patch_size == 2
    assert [(h // 2) * (w // 2) for h, w in sizes] == [60, 64, 24]
    xs = [torch.from_numpy(g[f"x{b}"]) for b in range(half)]
    t, cap, mask = torch.from_numpy(g["t"]), torch.from_numpy(g["cap"]), torch.from_numpy(g["mask"])
    scale = float(g["cfg_scale"])
    for key, kw in (("", {}), ("prop", dict(proportional_attn=True, base_seqlen=16))):
        ys = O.forward_packed(sd, cfg, xs + xs, t, cap, mask, **kw)
        for b, y in enumerate(ys):
            ref = torch.from_numpy(g[f"fwd{key}{b}"])
            assert tuple(y.shape) == (cfg.in_channels,) + sizes[b % half]
            assert float((y - ref).norm() / ref.norm()) < PACKED_TOL, (key, b)
        for b, y in enumerate(ys):  # model.py:908-913 per sample
            cond, unc = ys[b % half][:3], ys[b % half + half][:3]
            guided = torch.cat([unc + scale * (cond - unc), y[3:]], dim=0)
            ref = torch.from_numpy(g[f"cfg{key}{b}"])
            assert float((guided - ref).norm() / ref.norm()) < PACKED_TOL, (key, b)
            other = torch.from_numpy(g[f"cfg{key}{(b + half) % (2 * half)}"])
            assert torch.equal(ref[:3], other[:3]) and not torch.equal(ref[3], other[3])  # guided channels shared, channel 3 each row's own
    # the padded length is what the proportional scale sees: the short sample moves when it is packed
    assert not np.allclose(g["fwd2"], g["fwdprop2"], atol=1e-4)


def _table(sizes, Cc, patch):
    lib = _lib.load()
    hw = (C.c_int32 * (2 * len(sizes)))(*[v for s in sizes for v in s])
    tab, elems, nmax = (C.c_int32 * 320)(), C.c_int64(-1), C.c_int32(-1)
    rc = lib.lt_op_packed_table(hw, len(sizes), Cc, patch, tab, C.byref(elems), C.byref(nmax))
    return rc, np.array(tab[:], dtype=np.int64).reshape(5, 64), elems.value, nmax.value


def test_packed_table_matches_a_python_restatement():
    rng = np.random.default_rng(0)
    for trial in range(40):
        B = 64 if trial < 3 else int(rng.integers(1, 65))
        patch = int(rng.choice([1, 2, 4]))
        Cc = int(rng.choice([1, 4, 16]))
        sizes = [(patch * int(rng.integers(1, 40)), patch * int(rng.integers(1, 40))) for _ in range(B)]
        rc, tab, elems, nmax = _table(sizes, Cc, patch)
        assert rc == 0, _lib.load().lt_last_error()
        off = 0
        for b, (h, w) in enumerate(sizes):
            assert tab[:, b].tolist() == [off, h, w, (h // patch) * (w // patch), w // patch], (trial, b)
            off += Cc * h * w
        assert not tab[:, B:].any()
        assert elems == off and nmax == max((h // patch) * (w // patch) for h, w in sizes)


def test_packed_table_refusals():
    lib = _lib.load()
    for sizes, B, patch, word in (([(16, 16)] * 65, 65, 2, b"outside 1..64"), ([(16, 15)], 1, 2, b"multiple of the patch size"),
                                  ([(0, 16)], 1, 2, b"multiple of the patch size"), ([(-2, 16)], 1, 2, b"multiple of the patch size"),
                                  ([(16, 16)], 0, 2, b"outside 1..64"), ([(8190, 8190)] * 9, 9, 2, b"2^31")):
        hw = (C.c_int32 * (2 * len(sizes)))(*[v for s in sizes for v in s])
        tab = (C.c_int32 * 320)()
        assert lib.lt_op_packed_table(hw, B, 4, patch, tab, None, None) != 0
        assert word in lib.lt_last_error(), (sizes[:2], lib.lt_last_error())
    assert lib.lt_op_packed_table(None, 1, 4, 2, (C.c_int32 * 320)(), None, None) != 0 and b"null argument" in lib.lt_last_error()


def test_new_abi_calls_refuse_null_arguments():
    lib = _lib.load()
    a = _lib.LtStepArgs(batch=2, io_dtype=_lib.LT_BF16)
    hw = (C.c_int32 * 4)(16, 16, 16, 16)
    grid = (C.c_float * 2)(0.0, 1.0)
    one = C.c_void_p(64)  # never dereferenced: the engine pointer is null
    assert lib.lt_forward_cfg_packed(None, one, hw, one, one, C.byref(a), None) != 0
    assert b"lt_forward_cfg_packed: null argument" in lib.lt_last_error()
    assert lib.lt_sample_ode_packed(None, one, hw, None, one, grid, 2, 0, 1, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_packed: null argument" in lib.lt_last_error()
    for name in ("lt_forward_cfg_packed", "lt_sample_ode_packed", "lt_op_packed_table", "lt_op_patchify_packed", "lt_op_fill_pad_packed",
                 "lt_op_unpatchify_packed"):
        assert name in _lib.declared_symbols() and hasattr(lib, name)
