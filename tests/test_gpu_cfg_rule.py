"""GPU: rescaled and norm-limited guidance - lt_sample_ode_cfg_rule / lt_forward_cfg_rule.  Everything but the sums is exact.

* kernels: the partial sums of lt_op_guidance_stats equal torch's float64 sums within ``n 2^-52 sum |term|`` (every partial is a float64 sum of
  at most n terms in some order; so is torch's), and nothing behind them is written; lt_op_unpatchify_cfg_rule equals
  ``transport.guidance.guided_rule`` word for word, factors included, at every scale and rule, and the rule-off / dup forms equal
  lt_op_unpatchify_cfg_dev;
* loop: the engine's trajectory equals the host loop ``sample_cfg_rule`` around the same model at every slot; the (0, inf) call through the C
  entry is lt_sample_ode_cfg_schedule's trajectory; ``forward_with_cfg_rule`` is ``guided_rule(model.forward(...))``;
* graph path: two keys whatever the table, the blend and the limit hold;
* a class-conditional family and Flag-DiT through ``ODE.sample``; refusals by name; the ``sample.py`` driver."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import EngineLimits
from lumina_t2x_amd.transport import Sampler, create_transport
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

from gpu_util import P, lib, stream
from test_gpu_cfg_schedule import _grid, _tables
from test_gpu_sde import _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
INF = math.inf
_CACHE = {}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
def _rows(B, H, W, eol, seed, Cc=4, out_ch=8, p=2, device="cuda"):
    """final-layer rows [B Hp stride, ld] whose uncond samples are scaled by 0.25, 1, 4 - and the model output o [B, C, H, W] they hold"""
    Hp, Wp = H // p, W // p
    stride = Wp + eol
    ld = p * p * out_ch + 8
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(B, Hp * stride, ld, generator=g).mul(3)
    half = B // 2
    rows[half:] *= torch.tensor([(0.25, 1.0, 4.0)[b % 3] for b in range(half)]).view(-1, 1, 1)
    rows = rows.reshape(B * Hp * stride, ld).to(device, torch.bfloat16)
    o = rows.view(B, Hp, stride, ld)[:, :, :Wp, :p * p * out_ch].reshape(B, Hp, Wp, p, p, out_ch)
    o = o.permute(0, 5, 1, 3, 2, 4).reshape(B, out_ch, H, W)[:, :Cc].contiguous()  # (pH, pW, C_out) per token -> [B, C, H, W]
    return rows, o, stride, ld


def _ratios(o, w, ch, phi):
    """fr |g| / |c| per sample, from the reference's own factors: a norm limit below a sample's ratio scales that sample"""
    parts = []
    G.guided_rule(o, w, ch, phi, INF, parts)
    half = o.shape[0] // 2
    c, u = o[:half, :ch], o[half:, :ch]
    g = u + w * (c - u)
    norm = lambda t: t.double().reshape(half, -1).norm(dim=1)  # noqa: E731
    return [fr * float(x) for (fr, _), x in zip(parts, norm(g) / norm(c))]


def _f32(x):
    return float(np.float32(x))


KERNEL_SHAPES = [(2, 6, 10), (6, 6, 10), (2, 2, 2), (6, 2, 2)]  # 6 x 10: a non-square grid, slices of 6 or 8 elements; 2 x 2: 12 / 16 elements, empty slices


@pytest.mark.parametrize("eol", [0, 1], ids=["grid", "eol"])
@pytest.mark.parametrize("B,H,W", KERNEL_SHAPES)
def test_stats_partials_sum_to_the_float64_sums_and_write_nothing_else(B, H, W, eol):
    L = lib()
    S = L.lt_op_guidance_slices()
    assert S == 32
    half = B // 2
    rows, o, stride, ld = _rows(B, H, W, eol, seed=40 + B + H + eol)
    sentinel = -7.25
    for ch in (3, 4):
        n = ch * H * W
        for scale in (0.0, 4.0, 7.5, -1.5):
            parts = torch.full((half * S * 4 + 16,), sentinel, dtype=torch.float64, device="cuda")
            sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
            rc = L.lt_op_guidance_stats(P(rows), ld, B, 8, H, W, 2, P(sc), ch, stride if eol else 0, P(parts), stream())
            assert rc == 0, L.lt_last_error()
            assert bool((parts[half * S * 4:] == sentinel).all()) and not bool((parts[: half * S * 4] == sentinel).any())
            got = parts[: half * S * 4].view(half, S, 4)
            if n < S:  # one element per slice: the slices behind the last element hold zeros
                assert bool((got[:, n:] == 0).all())
            got = got.sum(1).cpu()
            c, u = o[:half, :ch], o[half:, :ch]
            g = u + scale * (c - u)
            cd, gd = c.double().reshape(half, -1), g.double().reshape(half, -1)
            for k, term in enumerate((cd, cd * cd, gd, gd * gd)):
                want, mag = term.sum(1).cpu(), term.abs().sum(1).cpu()
                err = (got[:, k] - want).abs()
                print(f"B {B} {H}x{W} eol {eol} ch {ch} scale {scale} sum {k}: err {err.tolist()} bound {(n * 2.0 ** -52 * mag).tolist()}")
                assert bool((err <= n * 2.0 ** -52 * mag).all()), (ch, scale, k, err.tolist(), mag.tolist())


@pytest.mark.parametrize("eol", [0, 1], ids=["grid", "eol"])
@pytest.mark.parametrize("B,H,W", KERNEL_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_rule_kernel_equals_guided_rule_word_for_word(dtype, B, H, W, eol):
    L = lib()
    S = L.lt_op_guidance_slices()
    Cc, half = 4, B // 2
    rows, o, stride, ld = _rows(B, H, W, eol, seed=60 + B + H + eol)
    n = B * Cc * H * W
    code = _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32
    sentinel = 1.5
    ws = stride if eol else 0

    def dev(scale, ch, dup):
        out = torch.full((n + 64,), sentinel, dtype=dtype, device="cuda")
        sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
        rc = L.lt_op_unpatchify_cfg_dev(P(rows), ld, P(out), code, B, Cc, 8, H, W, 2, 1, P(sc), ch, ws, dup, stream())
        assert rc == 0, L.lt_last_error()
        return out

    def rule(scale, ch, phi, r, dup=0):
        out = torch.full((n + 64,), sentinel, dtype=dtype, device="cuda")
        f = torch.full((half + 8,), sentinel, dtype=torch.float32, device="cuda")
        parts = torch.zeros(half * S * 4, dtype=torch.float64, device="cuda")
        sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
        pr = torch.tensor([phi, r], dtype=torch.float32, device="cuda")
        if not dup:
            assert L.lt_op_guidance_stats(P(rows), ld, B, 8, H, W, 2, P(sc), ch, ws, P(parts), stream()) == 0, L.lt_last_error()
        rc = L.lt_op_unpatchify_cfg_rule(P(rows), ld, P(out), code, B, Cc, 8, H, W, 2, 1, P(sc), ch, ws, dup, P(parts), P(pr), P(pr[1:]), P(f), stream())
        assert rc == 0, L.lt_last_error()
        assert bool((out[n:] == sentinel).all()) and bool((f[half:] == sentinel).all())
        return out, f[:half]

    for ch in (3, 4):
        for scale in (0.0, 4.0, 7.5, -1.5):
            rules = [(0.0, INF), (0.7, INF)]
            q0, q1 = _ratios(o, scale, ch, 0.0), _ratios(o, scale, ch, 1.0)
            if half > 1:  # r_mid, between the samples' ratios: some are limited, some are not (under full rescale every ratio is near 1: its own)
                assert min(q0) * 1.05 < max(q0), q0
                r_mid = _f32(math.sqrt(min(q0) * max(q0)))
                rules += [(0.0, r_mid), (1.0, r_mid), (1.0, _f32(sorted(q1)[half // 2]))]
            else:  # one sample: a limit below its ratio and one above
                rules += [(0.0, _f32(q0[0] * 0.5)), (1.0, _f32(q1[0] * 0.5)), (1.0, _f32(q0[0] * 2.0))]
            for phi, r in rules:
                tag = (dtype, B, H, W, eol, ch, scale, phi, r)
                parts = []
                want, fw = G.guided_rule(o, scale, ch, phi, r, parts)
                if half > 1 and (phi, r) == (0.0, r_mid):
                    assert any(fl < 1.0 for _, fl in parts) and any(fl == 1.0 for _, fl in parts), tag + (parts,)
                if half == 1 and r < q0[0]:
                    assert parts[0][1] < 1.0, tag + (parts,)
                got, f = rule(scale, ch, phi, r)
                assert torch.equal(_bits(f), _bits(fw)), tag + (f.tolist(), fw.tolist())
                assert torch.equal(_bits(got[:n]), _bits(want.to(dtype).reshape(-1))), tag
                if (phi, r) == (0.0, INF):
                    assert f.tolist() == [1.0] * half and torch.equal(_bits(got), _bits(dev(scale, ch, 0))), tag
        got, f = rule(4.0, ch, 0.7, 1.0, dup=1)
        assert torch.equal(_bits(got), _bits(dev(4.0, ch, 1))) and bool((f == sentinel).all()), (dtype, B, H, W, eol, ch)


# ---- loop ----------------------------------------------------------------------------------------------------------------------------
def _next(golden_dir):
    if "next" not in _CACHE:
        model, z, kw = _model(golden_dir, "next")
        _CACHE["next"] = (model, kw)
    return _CACHE["next"]


PHI, R = 0.7, 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    step_kw = dict(proportional_attn=True, base_seqlen=16)
    tgrid = _grid(method)
    n = (len(tgrid) - 1) * STAGES[method]
    g = torch.Generator().manual_seed(6)
    L = lib()
    for B, H, W in ((2, 16, 16), (4, 16, 24)):
        Bh = B // 2
        z = torch.randn(Bh, 4, H, W, generator=g).to("cuda", dtype).repeat(2, 1, 1, 1)
        cf, cm = (cap, cmask) if B == 2 else (torch.cat([cap, cap.flip(0)]), torch.cat([cmask, cmask.flip(0)]))
        t0 = torch.full((B,), 0.25, device="cuda")
        model.forward_with_cfg(z, t0, cf, cm, 4.0, **step_kw)  # the flags a plain forward reads
        tabs = _tables(tgrid, method)
        for name in ("interval", "ramp"):
            table = tabs[name]
            tag = (method, dtype, B, name)
            off = model.sample_ode_cfg_schedule(z, tgrid, table, cf, cm, method=method, return_trajectory=True, **step_kw)
            got = model.sample_ode_cfg_schedule(z, tgrid, table, cf, cm, method=method, return_trajectory=True, rescale=PHI, norm_limit=R, **step_kw)
            eng = model._engine
            G_, C_ = int((table != 1).sum()), int((table == 1).sum())
            assert eng.last_nfe() == n and eng.last_eval_rows() == B * G_ + Bh * C_, tag + (eng.last_nfe(), eng.last_eval_rows())
            final = model.sample_ode_cfg_schedule(z, tgrid, table, cf, cm, method=method, rescale=PHI, norm_limit=R, **step_kw)
            # the rule call at (0, inf) through the C entry: other kernels, the schedule call's states
            ident = eng.sample_ode_cfg_rule(z, tgrid, table, method, rescale=0.0, norm_limit=INF, **step_kw)
            parts = []
            want = G.sample_cfg_rule(model, z, tgrid, table, method, rescale=PHI, norm_limit=R, parts=parts, cap_feats=cf, cap_mask=cm, **step_kw)
            assert len(parts) == G_ * Bh and any(fl < 1.0 for _, fl in parts), tag + (parts,)  # the limit engages at some stage
            assert got.shape == want.shape == (len(tgrid),) + tuple(z.shape) and got.dtype == dtype, tag
            assert bool(torch.isfinite(want.float()).all()), tag
            for i in range(len(tgrid)):
                assert torch.equal(got[i], want[i]), tag + (i, int((got[i] != want[i]).sum()))
            assert torch.equal(final, got[-1]), tag
            assert not torch.equal(got[-1], off[-1]), tag
            assert torch.equal(ident, off), tag
        # one evaluation: guided_rule on the model's output of all rows
        for w, phi, r in ((4.0, PHI, R), (7.5, 1.0, INF), (1.0, 0.0, 0.5)):
            o = model.forward(torch.cat([z[:Bh]] * 2), t0, cf, cm)
            want, _ = G.guided_rule(o, w, 3, phi, r)
            got = model.forward_with_cfg_rule(z, t0, cf, cm, w, rescale=phi, norm_limit=r, **step_kw)
            assert got.dtype == dtype and torch.equal(got, want), (method, dtype, B, w, phi, r)
        assert torch.equal(model.forward_with_cfg_rule(z, t0, cf, cm, 4.0, **step_kw), model.forward_with_cfg(z, t0, cf, cm, 4.0, **step_kw))


def test_graph_path_replays_two_keys_whatever_the_scales_and_the_rule(golden_dir):
    model, _, kw = _model(golden_dir, "next")  # a fresh engine: no key has been used
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    step_kw = dict(proportional_attn=True, base_seqlen=16)
    H, W = 50, 82  # 25 x 41 = 1025 tokens: the smallest latent whose B' = 1 evaluation has more than 1024 rows
    tgrid = _grid("midpoint")
    table = torch.tensor([1.0, 2.0, 1.0, 3.0, 3.5, 1.0, 4.5, 5.0])
    G_, C_ = 5, 3
    z = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(8)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), cap, cmask, 4.0, **step_kw)  # engine, weights, prompt
    eng = model._engine
    before = eng.graph_replays()
    got = model.sample_ode_cfg_schedule(z, tgrid, table, cap, cmask, method="midpoint", return_trajectory=True, rescale=PHI, norm_limit=R, **step_kw)
    # the first use of a key runs eagerly, every later one replays: neither the scale nor the rule's parameters are part of the key
    assert eng.graph_replays() - before == (G_ - 1) + (C_ - 1)
    assert eng.last_nfe() == 8 and eng.last_eval_rows() == 2 * G_ + C_
    want = G.sample_cfg_rule(model, z, tgrid, table, "midpoint", rescale=PHI, norm_limit=R, cap_feats=cap, cap_mask=cmask, **step_kw)
    for i in range(len(tgrid)):
        assert torch.equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    # another blend and another limit: no new key - every evaluation replays - and another result, the host loop's
    before = eng.graph_replays()
    got2 = model.sample_ode_cfg_schedule(z, tgrid, table, cap, cmask, method="midpoint", return_trajectory=True, rescale=0.3, norm_limit=2.0, **step_kw)
    assert eng.graph_replays() - before == G_ + C_
    want2 = G.sample_cfg_rule(model, z, tgrid, table, "midpoint", rescale=0.3, norm_limit=2.0, cap_feats=cap, cap_mask=cmask, **step_kw)
    assert torch.equal(got2, want2) and not torch.equal(got2[-1], got[-1])


@pytest.mark.parametrize("family", ["imagenet", "flag"])
def test_other_families_run_the_same_call_through_the_transport_front_end(golden_dir, family):
    model, z, kw = _model(golden_dir, family)
    z = z.to("cuda", torch.bfloat16)
    assert z.shape[0] == 2 and z.shape[1] > 3  # guidance on 3 of more channels
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), **kw)  # the flags a plain forward reads
    o = ODE(5, "midpoint", 4)
    table = torch.tensor([1.0, 1.0, 2.0, 1.0, 4.0, 3.0, 1.0, 1.0])
    got = o.sample(z, model.forward_with_cfg, cfg_table=table, cfg_rescale=PHI, cfg_norm_limit=R, **kw)
    assert model._engine.last_nfe() == 8 and model._engine.last_eval_rows() == 2 * 3 + 5
    off = o.sample(z, model.forward_with_cfg, cfg_table=table, **kw)
    o.use_engine = False
    want = o.sample(z, model.forward_with_cfg, cfg_table=table, cfg_rescale=PHI, cfg_norm_limit=R, **kw)
    assert got.shape == (5,) + tuple(z.shape) and bool(torch.isfinite(want.float()).all())
    for i in range(5):
        assert torch.equal(got[i], want[i]), (family, i)
    assert not torch.equal(got[-1], off[-1])
    # without a table: cfg_scale at every stage, on the engine and on the host
    o.use_engine = True
    const = o.sample(z, model.forward_with_cfg, cfg_rescale=PHI, **kw)
    assert model._engine.last_nfe() == 8 and model._engine.last_eval_rows() == 16
    o.use_engine = False
    assert torch.equal(const, o.sample(z, model.forward_with_cfg, cfg_rescale=PHI, **kw))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    n = 2 * 4 * 16 * 16
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    lim = model.engine_limits  # room for a batch of 3: the odd batch must reach its own refusal
    model.engine_limits = EngineLimits(max(lim.max_batch, 6), lim.max_tokens, lim.max_text)
    t = torch.full((2,), 0.5, device="cuda")
    ref = model.forward_with_cfg(z, t, cap, cmask, 4.0)  # engine, weights, a prompt of 2 rows
    eng, L = model._engine, lib()
    out = torch.full((8 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    grid = (C.c_float * 3)(0.0, 0.5, 1.0)
    good = (C.c_float * 2)(4.0, 1.0)
    nan = float("nan")

    def traj(*, phi=0.5, r=1.0, batch=2, tab=good, ng=3, method=0):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        return L.lt_sample_ode_cfg_rule(eng.handle, P(z), P(out), P(out[4 * n:]), grid, ng, method, tab, phi, r, 1, C.byref(a), stream())

    def one(*, phi=0.5, r=1.0, batch=2, scale=4.0):
        a = eng._step_args(z, scale, 1.0, 1.0, None, False)
        a.batch = batch
        return L.lt_forward_cfg_rule(eng.handle, P(z), P(t), P(out), phi, r, C.byref(a), stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    for call, who in ((traj, "lt_sample_ode_cfg_rule:"), (one, "lt_forward_cfg_rule:")):
        refused(call(phi=1.5), who, "rescale")
        refused(call(phi=nan), who, "rescale")
        refused(call(phi=-0.25), who, "rescale")
        refused(call(r=0.0), who, "norm_limit")
        refused(call(r=-2.0), who, "norm_limit")
        refused(call(r=nan), who, "norm_limit")
        refused(call(batch=3), who, "even batch")
    refused(traj(tab=(C.c_float * 2)(4.0, nan)), "lt_sample_ode_cfg_rule:", "not finite")
    refused(traj(ng=1), "lt_sample_ode_cfg_rule:", "2 grid points")
    refused(traj(method=7), "lt_sample_ode_cfg_rule:", "unknown method")
    refused(traj(tab=None), "lt_sample_ode_cfg_rule:", "null argument")
    refused(one(scale=nan), "lt_forward_cfg_rule:", "not finite")
    eng.prepare_prompt_regional(cap, cmask, cap[:1].contiguous(), cmask[:1].contiguous(), 1, 1)
    refused(traj(), "lt_sample_ode_cfg_rule:", "regional prompt")
    refused(one(), "lt_forward_cfg_rule:", "regional prompt")
    eng.prepare_prompt(cap, cmask)
    # the Python layers refuse the same parameters, and a packed batch, before any engine call
    with pytest.raises(_lib.LuminaLibError, match="rescale"):
        eng.sample_ode_cfg_rule(z, [0.0, 0.5, 1.0], [4.0, 4.0], "euler", rescale=1.5)
    with pytest.raises(_lib.LuminaLibError, match="norm_limit"):
        model.forward_with_cfg_rule(z, t, cap, cmask, 4.0, norm_limit=0.0)
    with pytest.raises(_lib.LuminaLibError, match="packed"):
        model.forward_with_cfg_rule([z[0], z[1]], t, cap, cmask, 4.0, rescale=0.5)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # ... and the same arguments untouched are served; forward_with_cfg goes on as before
    assert traj() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:3 * n].float()).all()) and eng.last_nfe() == 2 and eng.last_eval_rows() == 3
    assert one() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:n].float()).all())
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0), ref)


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_sample_driver_with_a_rule_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_rule_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_rule_test"] = ctor
    (tmp_path / "prompts.txt").write_text("a red cube\n")
    gen = torch.Generator().manual_seed(3)
    table = {c: torch.randn(16, cfg.cap_feat_dim, generator=gen) for c in ("a red cube", "")}

    def encode(caps):
        feats = torch.stack([table[c] for c in caps]).to("cuda", torch.bfloat16)
        mask = torch.ones(len(caps), 16, dtype=torch.int64, device="cuda")
        mask[-1, 8:] = 0
        return feats, mask

    decoded = []

    def decode(lat):
        decoded.append(lat.clone())
        return torch.sigmoid(lat[:, :3].float())

    argv = ["--ckpt", str(ck), "--caption_path", str(tmp_path / "prompts.txt"), "--resolution", "256:128x128", "--num_sampling_steps", "5",
            "--sampling-method", "midpoint", "--time_shifting_factor", "4", "--seed", "11"]
    runs = {}
    try:
        for name, extra in (("default", []), ("rule", ["--cfg_rescale", "0.7", "--cfg_norm_limit", "1.0"]),
                            ("interval", ["--cfg_rescale", "0.7", "--cfg_norm_limit", "1.0", "--cfg_interval", "0.1", "0.8"])):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            runs[name] = (built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
    finally:
        del models.__dict__["NextDiT_tiny_rule_test"]
    fn = Sampler(create_transport()).sample_ode(sampling_method="midpoint", num_steps=5, time_shifting_factor=4.0)
    tgrid = fn.__self__.t
    itab = G.cfg_table(tgrid, "midpoint", 4.0, interval=(0.1, 0.8))
    Gi, Ci = int((itab != 1).sum()), int((itab == 1).sum())
    # every evaluation of a run lies in ONE whole-trajectory call
    assert runs == {"default": (8, 16), "rule": (8, 16), "interval": (8, 2 * Gi + Ci)}
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    feats, mask = encode(["a red cube", ""])
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    # the default invocation is the call it was
    want = fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1]
    assert torch.equal(decoded[0], want / 0.13025)
    phi = float(np.float32(0.7))
    want = model.sample_ode_cfg_schedule(z, tgrid, G.cfg_table(tgrid, "midpoint", 4.0), feats, mask, method="midpoint", rescale=phi, norm_limit=1.0, **kw)[:1]
    assert bool(torch.isfinite(decoded[1].float()).all()) and torch.equal(decoded[1], want / 0.13025) and not torch.equal(decoded[1], decoded[0])
    want = model.sample_ode_cfg_schedule(z, tgrid, itab, feats, mask, method="midpoint", rescale=phi, norm_limit=1.0, **kw)[:1]
    assert torch.equal(decoded[2], want / 0.13025) and not torch.equal(decoded[2], decoded[1])
