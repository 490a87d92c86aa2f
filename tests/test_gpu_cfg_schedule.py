"""GPU: guidance schedules - lt_sample_ode_cfg_schedule.  Everything is exact: no tolerance.

* kernel: lt_op_unpatchify_cfg_dev equals lt_op_unpatchify_cfg word for word at every scale, and with dup both halves are the plain
  unpatchify of the B' rows;
* loop: the engine's trajectory equals the host loop ``transport.guidance.sample_cfg_schedule`` around the same model at every slot, with the
  evaluation and row counts the table implies;
* identities: a constant table is lt_sample_ode at that scale, an all-ones table is lt_sample_ode without guidance on the cond rows, twice;
* graph path: one trajectory with five distinct scales and three conditional-only stages replays all but the first use of its TWO keys;
* a class-conditional family and Flag-DiT through ``ODE.sample(cfg_table=)``; refusals by name; the ``sample.py`` driver."""
import ctypes as C
import json
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
from test_gpu_sde import _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
_CACHE = {}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- kernel --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eol", [0, 1], ids=["grid", "eol"])
@pytest.mark.parametrize("B", [2, 6])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_kernel_equals_the_host_scale_kernel_word_for_word(dtype, B, eol):
    L = lib()
    Cc, out_ch, H, W, p = 4, 8, 6, 10, 2  # 3 x 5 tokens: a non-square grid; 480 / 1440 elements: several blocks, the last one partial
    Hp, Wp = H // p, W // p
    stride = Wp + eol  # Flag-DiT: one eol column per token row, skipped
    ld = p * p * out_ch + 8
    g = torch.Generator().manual_seed(17 + B + eol)
    rows = torch.randn(B * Hp * stride, ld, generator=g).mul(3).to("cuda", torch.bfloat16)
    n = B * Cc * H * W
    code = _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32
    sentinel = 1.5

    def buf():
        return torch.full((n + 64,), sentinel, dtype=dtype, device="cuda")

    def host(use_cfg, scale, ch, src=rows, b=B):
        out = buf()
        assert L.lt_op_unpatchify_cfg(P(src), ld, P(out), code, b, Cc, out_ch, H, W, p, use_cfg, scale, ch, stride if eol else 0, stream()) == 0
        return out

    def dev(use_cfg, scale, ch, dup):
        out = buf()
        sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
        rc = L.lt_op_unpatchify_cfg_dev(P(rows), ld, P(out), code, B, Cc, out_ch, H, W, p, use_cfg, P(sc), ch, stride if eol else 0, dup, stream())
        assert rc == 0, L.lt_last_error()
        return out

    for ch in (3, 4):
        for scale in (0.0, 1.0, 4.0, 7.5, -1.5):
            got, want = dev(1, scale, ch, 0), host(1, scale, ch)
            assert torch.equal(_bits(got), _bits(want)), (dtype, B, eol, ch, scale)
            assert bool((got[n:] == sentinel).all())
        assert torch.equal(_bits(dev(0, 4.0, ch, 0)), _bits(host(0, 4.0, ch)))
        # dup: the first B / 2 samples of the row buffer, unguided, in both halves of the output
        got = dev(1, 4.0, ch, 1)
        half = host(0, 1.0, ch, rows[: (B // 2) * Hp * stride], B // 2)[: n // 2]
        assert torch.equal(_bits(got[: n // 2]), _bits(half)) and torch.equal(_bits(got[n // 2:n]), _bits(half)), (dtype, B, eol, ch)
        assert bool((got[n:] == sentinel).all())


# ---- loop ----------------------------------------------------------------------------------------------------------------------------
def _next(golden_dir):
    if "next" not in _CACHE:
        model, z, kw = _model(golden_dir, "next")
        _CACHE["next"] = (model, kw)
    return _CACHE["next"]


def _grid(method):
    return ODE(9 if method == "euler" else 5, method, 4).t  # 8 stages for euler and midpoint, 16 for rk4


def _tables(tgrid, method):
    stages = STAGES[method]
    n = (len(tgrid) - 1) * stages
    ts = G.stage_times(tgrid, method, torch.float32, False)
    # guided in the middle, conditional-only on both sides; with more than one stage per step the interval opens INSIDE a step
    lo, hi = float(ts[stages + (1 if stages > 1 else 0)]), float(ts[-2])
    interval = G.cfg_table(tgrid, method, 4.0, interval=(lo, hi))
    assert float(interval[0]) == 1.0 and float(interval[-1]) == 1.0 and 0 < int((interval == 4.0).sum()) < n
    if stages > 1:
        assert float(interval[stages]) == 1.0 and float(interval[stages + 1]) == 4.0
    ramp = torch.tensor([1.5 + 0.5 * (i % 8) for i in range(n)])
    assert len(set(ramp.tolist())) == 8
    return {"interval": interval, "ramp": ramp, "fours": torch.full((n,), 4.0), "ones": torch.ones(n)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, method, dtype):
    model, kw = _next(golden_dir)
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    step_kw = dict(proportional_attn=True, base_seqlen=16)
    tgrid = _grid(method)
    stages = STAGES[method]
    n = (len(tgrid) - 1) * stages
    g = torch.Generator().manual_seed(6)
    for B, H, W in ((2, 16, 16), (4, 16, 24)):
        Bh = B // 2
        z = torch.randn(Bh, 4, H, W, generator=g).to("cuda", dtype).repeat(2, 1, 1, 1)
        cf, cm = (cap, cmask) if B == 2 else (torch.cat([cap, cap.flip(0)]), torch.cat([cmask, cmask.flip(0)]))
        model.forward_with_cfg(z, torch.zeros(B, device="cuda"), cf, cm, 4.0, **step_kw)  # the flags a plain forward reads
        # the identities' right-hand sides: lt_sample_ode with guidance at 4, and without guidance on the cond rows
        o = ODE(len(tgrid), method, 4)
        guided = o.sample(z, model.forward_with_cfg, cap_feats=cf, cap_mask=cm, cfg_scale=4.0, **step_kw)
        plain = o.sample(z[:Bh], model.forward, cap_feats=cf[:Bh].contiguous(), cap_mask=cm[:Bh].contiguous())
        for name, table in _tables(tgrid, method).items():
            tag = (method, dtype, B, name)
            got = model.sample_ode_cfg_schedule(z, tgrid, table, cf, cm, method=method, return_trajectory=True, **step_kw)
            eng = model._engine
            G_, C_ = int((table != 1).sum()), int((table == 1).sum())
            assert eng.last_nfe() == n and eng.last_eval_rows() == B * G_ + Bh * C_, tag + (eng.last_nfe(), eng.last_eval_rows())
            want = G.sample_cfg_schedule(model, z, tgrid, table, method, cap_feats=cf, cap_mask=cm, **step_kw)
            assert got.shape == want.shape == (len(tgrid),) + tuple(z.shape) and got.dtype == dtype, tag
            assert bool(torch.isfinite(want.float()).all()), tag
            for i in range(len(tgrid)):
                assert torch.equal(got[i], want[i]), tag + (i, int((got[i] != want[i]).sum()))
            final = model.sample_ode_cfg_schedule(z, tgrid, table, cf, cm, method=method, **step_kw)
            assert torch.equal(final, got[-1]), tag
            if name == "fours":
                assert torch.equal(got, guided), tag
            elif name == "ones":
                assert torch.equal(got[:, :Bh], plain) and torch.equal(got[:, Bh:], got[:, :Bh]), tag
            else:
                assert not torch.equal(got[-1], guided[-1]), tag
        # through the transport front end: the same call, and the host loop with use_engine = False
        table = _tables(tgrid, method)["interval"]
        via = o.sample(z, model.forward_with_cfg, cfg_table=table, cap_feats=cf, cap_mask=cm, cfg_scale=4.0, **step_kw)
        assert model._engine.last_nfe() == n and model._engine.last_eval_rows() < n * B
        o.use_engine = False
        assert torch.equal(via, o.sample(z, model.forward_with_cfg, cfg_table=table, cap_feats=cf, cap_mask=cm, cfg_scale=4.0, **step_kw))


def test_graph_path_replays_two_keys_whatever_the_scales(golden_dir):
    model, _, kw = _model(golden_dir, "next")  # a fresh engine: no key has been used
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    step_kw = dict(proportional_attn=True, base_seqlen=16)
    H, W = 50, 82  # 25 x 41 = 1025 tokens: the smallest latent whose B' = 1 evaluation has more than 1024 rows
    assert (H // 2) * (W // 2) == 1025
    tgrid = _grid("midpoint")
    table = torch.tensor([1.0, 2.0, 1.0, 3.0, 3.5, 1.0, 4.5, 5.0])
    G_, C_ = 5, 3
    z = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(8)).to("cuda", torch.bfloat16).repeat(2, 1, 1, 1)
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), cap, cmask, 4.0, **step_kw)  # engine, weights, prompt
    eng = model._engine
    before = eng.graph_replays()
    got = model.sample_ode_cfg_schedule(z, tgrid, table, cap, cmask, method="midpoint", return_trajectory=True, **step_kw)
    # the first use of a key runs eagerly, every later one replays: the scale is no part of the key
    assert eng.graph_replays() - before == (G_ - 1) + (C_ - 1)
    assert eng.last_nfe() == 8 and eng.last_eval_rows() == 2 * G_ + C_
    assert eng.get_option("layout_flips") >= 0
    want = G.sample_cfg_schedule(model, z, tgrid, table, "midpoint", cap_feats=cap, cap_mask=cmask, **step_kw)
    for i in range(len(tgrid)):
        assert torch.equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))


@pytest.mark.parametrize("family", ["imagenet", "flag"])
def test_other_families_run_the_same_call_through_the_transport_front_end(golden_dir, family):
    model, z, kw = _model(golden_dir, family)
    z = z.to("cuda", torch.bfloat16)
    assert z.shape[0] == 2
    model.forward_with_cfg(z, torch.zeros(2, device="cuda"), **kw)  # the flags a plain forward reads
    o = ODE(5, "midpoint", 4)
    table = torch.tensor([1.0, 1.0, 2.0, 1.0, 4.0, 3.0, 1.0, 1.0])
    got = o.sample(z, model.forward_with_cfg, cfg_table=table, **kw)
    assert model._engine.last_nfe() == 8 and model._engine.last_eval_rows() == 2 * 3 + 5
    o.use_engine = False
    want = o.sample(z, model.forward_with_cfg, cfg_table=table, **kw)
    assert got.shape == (5,) + tuple(z.shape) and bool(torch.isfinite(want.float()).all())
    for i in range(5):
        assert torch.equal(got[i], want[i]), (family, i)


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
    bad = (C.c_float * 2)(4.0, float("nan"))

    def call(*, tab=good, method=0, ng=3, batch=2, zz=P(z)):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        return L.lt_sample_ode_cfg_schedule(eng.handle, zz, P(out), P(out[4 * n:]), grid, ng, method, tab, 1, C.byref(a), stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    who = "lt_sample_ode_cfg_schedule:"
    refused(call(batch=3), who, "even batch")
    refused(call(tab=bad), who, "not finite")
    refused(call(ng=1), who, "2 grid points")
    refused(call(method=7), who, "unknown method")
    refused(call(method=-1), who, "unknown method")
    refused(call(tab=None), who, "null argument")
    refused(call(zz=C.c_void_p(0)), who, "null argument")
    refused(call(batch=0), "batch 0 outside")
    eng.prepare_prompt_regional(cap, cmask, cap[:1].contiguous(), cmask[:1].contiguous(), 1, 1)
    refused(call(), who, "regional prompt")
    with pytest.raises(_lib.LuminaLibError, match="entries"):
        eng.sample_ode_cfg_schedule(z, [0.0, 0.5, 1.0], [4.0], "euler")
    with pytest.raises(_lib.LuminaLibError, match="not in"):
        eng.sample_ode_cfg_schedule(z, [0.0, 1.0], [4.0], "heun2")
    # ... and the same arguments untouched are served, with the prompt prepared ONCE for both rows; forward_with_cfg goes on as before
    eng.prepare_prompt(cap, cmask)
    assert call() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:3 * n].float()).all()) and eng.last_nfe() == 2 and eng.last_eval_rows() == 3
    assert torch.equal(model.forward_with_cfg(z, t, cap, cmask, 4.0), ref)


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_sample_driver_with_a_guidance_interval_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample as S

    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_guidance_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_guidance_test"] = ctor
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
        for name, extra in (("default", []), ("interval", ["--cfg_interval", "0.1", "0.8"]), ("cosine", ["--cfg_schedule", "cosine"])):
            args = S.build_parser().parse_args(argv + extra + ["--image_save_path", str(tmp_path / name)])
            S.run(args, encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim, decode_fn=decode)
            runs[name] = (built[-1]._engine.last_nfe(), built[-1]._engine.last_eval_rows())
    finally:
        del models.__dict__["NextDiT_tiny_guidance_test"]
    fn = Sampler(create_transport()).sample_ode(sampling_method="midpoint", num_steps=5, time_shifting_factor=4.0)
    tgrid = fn.__self__.t
    # every evaluation of a run lies in ONE whole-trajectory call; the interval's conditional-only stages run one row
    itab = G.cfg_table(tgrid, "midpoint", 4.0, interval=(0.1, 0.8))
    Gi, Ci = int((itab != 1).sum()), int((itab == 1).sum())
    assert Gi > 0 and Ci > 0
    assert runs == {"default": (8, 16), "interval": (8, 2 * Gi + Ci), "cosine": (8, 16)}
    model = built[0]
    torch.manual_seed(11)
    z = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16).repeat(2, 1, 1, 1)
    feats, mask = encode(["a red cube", ""])
    kw = dict(proportional_attn=True, base_seqlen=256, scale_factor=1.0, scale_watershed=1.0)
    # the default invocation is the call it was
    want = fn(z, model.forward_with_cfg, cap_feats=feats, cap_mask=mask, cfg_scale=4.0, **kw)[-1][:1]
    assert torch.equal(decoded[0], want / 0.13025)
    want = model.sample_ode_cfg_schedule(z, tgrid, itab, feats, mask, method="midpoint", **kw)[:1]
    assert torch.equal(decoded[1], want / 0.13025) and not torch.equal(decoded[1], decoded[0])
    ctab = G.cfg_table(tgrid, "midpoint", 4.0, schedule=G.cosine_schedule(4.0, float(tgrid[0]), float(tgrid[-1])))
    want = model.sample_ode_cfg_schedule(z, tgrid, ctab, feats, mask, method="midpoint", **kw)[:1]
    assert torch.equal(decoded[2], want / 0.13025) and not torch.equal(decoded[2], decoded[0])
