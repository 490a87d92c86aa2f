"""CPU: prompt-driven editing - transport/edit.py (FlowEdit).  No GPU.  Everything is exact.

* both chains (``mix``, ``combine``) against their float64 restatement with explicit roundings (tests/exact_edit.py), word for word, at bf16 and
  fp32, on random operands and on operands that meet bf16 ties in ``w d``, in ``v_t - v_s`` and in the final sum;
* ``sample_flowedit`` around stub models: identical source and target conditioning with equal scales keeps ``x_src``; equal scales give rows
  0 / 1 of the ``forward_with_cfg`` expression on the same four rows; a constant-velocity stub ends on the closed form;
* ``flowedit_scales``; refusals; the driver's arguments and its flow with injected stages; the ABI declares, binds and documents the entries."""
import argparse
import json

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import edit as E
from lumina_t2x_amd.transport.mini import ODE

import exact_edit as X

DTYPES = [torch.bfloat16, torch.float32]
NEW = ("lt_sample_flowedit", "lt_op_flowedit_mix", "lt_op_flowedit_combine")


# ---- the chains ----------------------------------------------------------------------------------------------------------------------
def _random(dtype, Bp=2, C=4, H=5, W=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    x, w = (torch.randn(Bp, C, H, W, generator=g).to(dtype) for _ in range(2))
    z = (x.float() + 0.05 * torch.randn(Bp, C, H, W, generator=g)).to(dtype)
    out4 = torch.randn(4 * Bp, C, H, W, generator=g).mul(1.5).to(dtype)
    return x, z, w, out4


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_mix_equals_the_float64_restatement_word_for_word(dtype):
    R = X.rounding(dtype)
    grid = ODE(6, "euler", 4).t
    for x, z, w, t, t1 in [_random(dtype)[:3] + (float(grid[2]), float(grid[3])), X.mix_tie_operands(dtype) + (0.5,)]:
        tt, omt, _ = X.scalars(t, t1)
        zs, zt = E.mix(x, z, w, float(np.float32(t)))
        want_s, want_t = X.mix_chain(X.f64(x), X.f64(z), X.f64(w), tt, omt, R)
        assert zs.dtype == zt.dtype == dtype
        assert X.same_words(zs, want_s) and X.same_words(zt, want_t), (dtype, t)
        # the edit delta survives: zt - zs is z - x_src wherever that is exact, and z == x_src gives zt == zs bit for bit
        assert torch.equal(E.mix(x, x, w, float(np.float32(t)))[1], zs)
        assert torch.equal(E.edit_tail_start(z, x, w, float(np.float32(t))), zt)
    if dtype == torch.bfloat16:
        x, z, w, t = X.mix_tie_operands(dtype)
        assert X.bf16_ties(X.f64(x) * 0.375) > 16 and X.bf16_ties(X.f64(w) * 0.625) > 16
        # what the left-to-right form would lose: (z + zs) - x_src rounds the small delta away on some elements
        zs, zt = E.mix(x, z, w, t)
        assert not torch.equal((z + zs) - x, zt)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_combine_equals_the_float64_restatement_word_for_word(dtype):
    R = X.rounding(dtype)
    grid = ODE(6, "euler", 4).t
    _, _, dt = X.scalars(float(grid[2]), float(grid[3]))
    for ch in (3, 4, 1):
        for w_s, w_t in ((1.5, 5.5), (1.0, 1.0), (0.0, -2.25)):
            x, z, w, out4 = _random(dtype, seed=ch)
            got = E.combine(z, out4, w_s, w_t, float(grid[3]) - float(grid[2]), ch)
            parts = {}
            want = X.combine_chain(X.f64(z), X.f64(out4), w_s, w_t, dt, ch, R, parts)
            assert got.dtype == dtype and X.same_words(got, want), (dtype, ch, w_s, w_t)
            v_s, v_t = E.guided_pair(out4, w_s, w_t, ch)
            assert X.same_words(v_s, parts["v_s"]) and X.same_words(v_t, parts["v_t"])
    z, out4, w_s, w_t, dtf, ch = X.tie_operands(dtype)
    parts = {}
    want = X.combine_chain(X.f64(z), X.f64(out4), w_s, w_t, np.float64(dtf), ch, R, parts)
    assert X.same_words(E.combine(z, out4, w_s, w_t, dtf, ch), want), dtype
    # the operands do meet ties at the three roundings (counted on the exact float64 values, whatever the state dtype)
    assert X.bf16_ties(parts["wd"]) >= 32 and X.bf16_ties(parts["dv"]) >= 32 and X.bf16_ties(parts["total"]) >= 16, \
        [X.bf16_ties(parts[k]) for k in ("wd", "dv", "total")]


# ---- the host loop -------------------------------------------------------------------------------------------------------------------
class Toy:
    """plain forward of a conditional toy: the output depends on x, t and the row's conditioning vector"""

    def forward(self, x, t, y):
        s = y.to(x.dtype).reshape(-1, 1, 1, 1)
        return (x * 0.5 + s * torch.tanh(x) - t.to(x.dtype).reshape(-1, 1, 1, 1)).to(x.dtype)


def _setup(dtype, Bp=2, n=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Bp, 4, 6, 6, generator=g).to(dtype)
    noise = torch.randn(n, Bp, 4, 6, 6, generator=g).to(dtype)
    return x, noise, ODE(n + 1, "euler", 4).t


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_identical_conditioning_and_equal_scales_keep_the_source_exactly(dtype):
    x, noise, tgrid = _setup(dtype)
    y = torch.tensor([0.3, -0.7] * 2 + [0.1, 0.2] * 2)  # src == tgt rows, neg_src == neg_tgt rows
    out = E.sample_flowedit(Toy().forward, x, tgrid, noise, E.flowedit_scales(4, 3.5, 3.5), y=y)
    assert out.shape == (5,) + tuple(x.shape) and out.dtype == dtype
    for i in range(5):
        assert torch.equal(out[i], x), (dtype, i)
    # ... and another target moves it
    y2 = y.clone()
    y2[2:4] = torch.tensor([0.9, 0.4])
    assert not torch.equal(E.sample_flowedit(Toy().forward, x, tgrid, noise, E.flowedit_scales(4, 3.5, 3.5), y=y2)[-1], x)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_equal_scales_are_the_forward_with_cfg_expression_on_the_four_rows(dtype):
    x, noise, tgrid = _setup(dtype, Bp=1)
    y = torch.tensor([0.3, 0.9, 0.1, -0.2])
    vel = []
    w = 4.0
    states = E.sample_flowedit(Toy().forward, x, tgrid, noise, E.flowedit_scales(4, w, w), y=y, velocities=vel)
    assert len(vel) == 4
    for i in range(4):
        zs, zt = E.mix(x, states[i], noise[i], float(tgrid[i]))
        # forward_with_cfg (reference model.py:901-913) on the rows [zs, zt | zs, zt]: cond half, uncond half, channels [:3]
        o = Toy().forward(torch.cat([zs, zt, zs, zt]), torch.full((4,), float(tgrid[i])), y)
        eps, rest = o[:, :3], o[:, 3:]
        cond, unc = torch.split(eps, 2, dim=0)
        half = unc + w * (cond - unc)
        ref = torch.cat([torch.cat([half, half]), rest], 1)
        assert torch.equal(vel[i][0], ref[0:1]) and torch.equal(vel[i][1], ref[1:2]), (dtype, i)


def test_constant_velocity_stub_ends_on_the_closed_form():
    x, noise, _ = _setup(torch.float32, Bp=1, n=4)
    tgrid = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])  # dt exact
    vals = torch.tensor([2.0, 5.0, 1.0, 3.0])  # c_s, c_t, u_s, u_t

    def const(xx, t):
        return vals.reshape(4, 1, 1, 1).expand(4, *xx.shape[1:]).clone()

    w_s, w_t = 1.5, 2.0
    out = E.sample_flowedit(const, x, tgrid, noise, E.flowedit_scales(4, w_s, w_t))
    v_s, v_t = 1.0 + w_s * (2.0 - 1.0), 3.0 + w_t * (5.0 - 3.0)
    want = x.clone()
    want[:, :3] += v_t - v_s  # four steps of dt = 1 / 4, every value exact in fp32
    want[:, 3:] += 5.0 - 2.0  # the unguided channel takes the cond rows
    assert torch.allclose(out[-1], want, rtol=0, atol=4 * 2.0 ** -20)
    # on a source of small integers every step is exact: equality
    xi = torch.randint(-8, 8, x.shape).float()
    out = E.sample_flowedit(const, xi, tgrid, noise, E.flowedit_scales(4, w_s, w_t))
    want = xi.clone()
    want[:, :3] += v_t - v_s
    want[:, 3:] += 3.0
    assert torch.equal(out[-1], want)


# ---- scales and refusals -------------------------------------------------------------------------------------------------------------
def test_flowedit_scales():
    s = E.flowedit_scales(3, 1.5, 5.5)
    assert s.dtype == torch.float32 and s.tolist() == [[1.5, 5.5]] * 3 and s.is_contiguous()
    s = E.flowedit_scales(3, [1.0, 1.5, 2.0], torch.tensor([5.5, 4.5, 3.5], dtype=torch.float64))
    assert s.tolist() == [[1.0, 5.5], [1.5, 4.5], [2.0, 3.5]]
    with pytest.raises(ValueError, match="2 entries for 3 intervals"):
        E.flowedit_scales(3, [1.0, 2.0], 5.5)
    with pytest.raises(ValueError, match="not finite"):
        E.flowedit_scales(2, 1.5, [5.5, float("nan")])
    with pytest.raises(ValueError, match="at least one interval"):
        E.flowedit_scales(0, 1.5, 5.5)
    with pytest.raises(ValueError, match=r"\[3, 2\]"):
        E.check_scales(torch.zeros(3, 3), 3)


def test_refusals():
    x, noise, tgrid = _setup(torch.bfloat16)
    sc = E.flowedit_scales(4, 1.5, 5.5)
    y = torch.zeros(8)
    toy = Toy().forward
    for method in ("midpoint", "rk4", "abm2", "dopri5"):
        with pytest.raises(NotImplementedError, match="euler method only"):
            E.sample_flowedit(toy, x, tgrid, noise, sc, y=y, method=method)
    with pytest.raises(ValueError, match="multiple of 4"):  # conditioning for 6 rows: not 4 B'
        E.sample_flowedit(toy, x, tgrid, noise, sc, y=torch.zeros(6))
    with pytest.raises(ValueError, match="noise must be"):
        E.sample_flowedit(toy, x, tgrid, noise[:3], sc, y=y)
    with pytest.raises(ValueError, match="noise must be"):
        E.sample_flowedit(toy, x, tgrid, noise.float(), sc, y=y)
    with pytest.raises(ValueError, match="z must have"):
        E.sample_flowedit(toy, x, tgrid, noise, sc, y=y, z=x[:1])
    with pytest.raises(ValueError, match="z must have"):
        E.sample_flowedit(toy, x, tgrid, noise, sc, y=y, z=x.float())
    with pytest.raises(ValueError, match="unsupported"):
        E.check_edit_operands(x.half(), None, noise.half(), 4)
    with pytest.raises(ValueError, match=r"\[B', C, H, W\]"):
        E.check_edit_operands(x[0], None, noise, 4)
    with pytest.raises(ValueError, match="2 grid points"):
        E.sample_flowedit(toy, x, tgrid[:1], noise[:0], sc[:0], y=y)
    with pytest.raises(ValueError, match=r"\[4, 2\]"):
        E.sample_flowedit(toy, x, tgrid, noise, sc[:3], y=y)
    with pytest.raises(TypeError, match="step flags"):
        E.edit(Toy(), x, tgrid, noise, (y,), 1.5, 5.5, proportional_attn=True)
    # the front end on a model that is not engine-backed is the host loop
    got = E.edit(Toy(), x, tgrid, noise, (y,), 1.5, 5.5, return_trajectory=True)
    assert torch.equal(got, E.sample_flowedit(toy, x, tgrid, noise, sc, y=y))


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_driver_arguments_and_grids():
    from lumina_t2x_amd import sample_edit as S
    p = S.build_parser()
    a = p.parse_args(["--ckpt", "x", "--image", "in.png", "--source_caption", "a cat"])
    assert (a.src_cfg, a.tgt_cfg, a.n_min, a.negative_caption, a.seed) == (1.5, 5.5, 0, "", 0)
    with pytest.raises(SystemExit):
        p.parse_args(["--ckpt", "x", "--image", "in.png"])  # no source caption
    full = ODE(10, "euler", 4.0, strength=0.6).t
    grid, edit, tail = S.edit_grids(10, 4.0, 0.6, 0)
    assert torch.equal(grid, full) and torch.equal(edit, full) and tail is None and len(full) == 6
    grid, edit, tail = S.edit_grids(10, 4.0, 0.6, 2)
    assert torch.equal(edit, full[:4]) and torch.equal(tail, full[3:]) and float(edit[-1]) == float(tail[0])
    with pytest.raises(ValueError, match="n_min"):
        S.edit_grids(10, 4.0, 0.6, 5)
    with pytest.raises(ValueError, match="n_min"):
        S.edit_grids(10, 4.0, 0.6, -1)
    with pytest.raises(ValueError, match="no interval"):
        S.edit_grids(10, 4.0, 0.05, 0)


class ToyT2I:
    """a model that is not engine-backed: plain forward and forward_with_cfg of a caption-conditional toy"""

    def forward(self, x, t, cap_feats, cap_mask):
        s = (cap_feats.float() * cap_mask[..., None]).mean((1, 2)).to(x.dtype).reshape(-1, 1, 1, 1)
        return (x * 0.25 + s - t.to(x.dtype).reshape(-1, 1, 1, 1)).to(x.dtype)

    def forward_with_cfg(self, x, t, cap_feats, cap_mask, cfg_scale, **kw):
        half = x[: len(x) // 2]
        o = self.forward(torch.cat([half, half]), t, cap_feats, cap_mask)
        cond, unc = torch.split(o[:, :3], len(x) // 2, dim=0)
        g = unc + cfg_scale * (cond - unc)
        return torch.cat([torch.cat([g, g]), o[:, 3:]], 1)


def test_driver_with_injected_stages_runs_the_host_loop(tmp_path):
    from lumina_t2x_amd import sample_edit as S
    dev = "cuda" if torch.cuda.is_available() else "cpu"  # the driver's own choice; the toy model runs the host loop on either
    ck = tmp_path / "ckpt"
    ck.mkdir()
    torch.save(argparse.Namespace(model="unused", qk_norm=True, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    (tmp_path / "targets.txt").write_text("a red cube\na blue ball\n")
    gen = torch.Generator().manual_seed(5)
    table = {c: torch.randn(8, 16, generator=gen) for c in ("a cube", "a red cube", "a blue ball", "")}
    seen = []

    def encode(caps):
        seen.append(list(caps))
        return torch.stack([table[c] for c in caps]).to(dev), torch.ones(len(caps), 8, dtype=torch.int64, device=dev)

    decoded = []

    def decode(lat):
        decoded.append(lat.clone())
        return torch.sigmoid(lat[:, :3].float())

    img = (torch.rand(3, 64, 64, generator=gen) * 2 - 1).to(dev)
    venc = lambda im: torch.nn.functional.avg_pool2d(im, 8)[:, [0, 1, 2, 0]]  # noqa: E731
    argv = ["--ckpt", str(ck), "--image", "unused.png", "--source_caption", "a cube", "--caption_path", str(tmp_path / "targets.txt"),
            "--resolution", "256:64x64", "--num_sampling_steps", "8", "--time_shifting_factor", "4", "--strength", "0.75", "--seed", "7",
            "--precision", "fp32", "--proportional_attn", "0"]
    model = ToyT2I()
    for name, extra in (("plain", []), ("tail", ["--n_min", "2"])):
        args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
        info = S.run(args, encode_fn=encode, cap_feat_dim=16, vae_encode_fn=venc, decode_fn=decode, model=model, image=img)
        assert len(info) == 2 and seen[-1] == ["a cube", "a blue ball", "", ""]
        rec = json.loads((tmp_path / name / "data.json").read_text())[0]
        assert (rec["src_cfg"], rec["tgt_cfg"], rec["strength"], rec["seed"], rec["intervals"]) == (1.5, 5.5, 0.75, 7, 5)
        assert rec["n_min"] == (2 if extra else 0) and rec["t_start"] == float(ODE(8, "euler", 4.0, strength=0.75).t[0])
    # the run without a tail is the host loop on the cut grid with the seed's draws
    grid = ODE(8, "euler", 4.0, strength=0.75).t
    torch.random.manual_seed(7)
    x_src = venc(img[None]) * 0.13025
    noise = torch.randn([5, 1, 4, 8, 8], device=dev)
    feats, mask = encode(["a cube", "a red cube", "", ""])
    want = E.sample_flowedit(model.forward, x_src, grid, noise, E.flowedit_scales(5, 1.5, 5.5), cap_feats=feats, cap_mask=mask)[-1]
    assert torch.equal(decoded[0], want / 0.13025)
    # with --n_min 2: three edit intervals, one more draw, then guided sampling of the target over the last two
    torch.random.manual_seed(7)
    noise = torch.randn([3, 1, 4, 8, 8], device=dev)
    z = E.sample_flowedit(model.forward, x_src, grid[:4], noise, E.flowedit_scales(3, 1.5, 5.5), cap_feats=feats, cap_mask=mask)[-1]
    start = E.edit_tail_start(z, x_src, torch.randn([1, 4, 8, 8], device=dev), float(grid[3]))
    tail = ODE(8, "euler", 4.0)
    tail.t = grid[3:]
    want = tail.sample(start.repeat(2, 1, 1, 1), model.forward_with_cfg, cap_feats=feats[[1, 3]], cap_mask=mask[[1, 3]], cfg_scale=5.5)[-1][:1]
    assert torch.equal(decoded[2], want / 0.13025) and not torch.equal(decoded[2], decoded[0])


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_documented():
    declared = set(_lib.declared_symbols())
    text = _lib.header_text(strip_comments=False)
    for name in NEW:
        assert name in declared and name in _lib._SIGNATURES, name
    assert len(_lib._SIGNATURES["lt_sample_flowedit"][1]) == 11
    for word in ("DESIGN.md 7l", "zt  = R(zs + R(z - x_src))", "z' = R(z + R(R(v_t - v_s) dt))", "multiple of 4", "n_avg"):
        assert word in text, word
