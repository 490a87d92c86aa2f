"""-m gpu: masked (inpainting) ODE sampling inside the engine - lt_sample_ode_masked / lt_sample_ode_masked_packed.

The reference has no inpainting sampler; the pin is the host loop of plain torch expressions (transport/masked.py: sample_masked) on the same
device, around the same engine-backed model:

* lt_op_ode_combine_masked against the torch expressions (tests/masked_torch.py), every output word compared as an integer;
* NextDiT.sample_ode_masked against sample_masked, torch.equal at every trajectory slot, bf16 and fp32 states, with and without guidance,
  square and rectangular latents, euler / midpoint / rk4 and a cut grid; mask = 1 everywhere is lt_sample_ode's trajectory, mask = 0
  everywhere ends on x1 bit for bit; the evaluation count is the plain call's;
* a class-conditional family through ODE.sample(mask=...) on one grid;
* the packed call against sample_masked around forward_with_cfg_packed on the flat state (the existing packed tests hold the packed sampler to
  exactly that loop, not to the tensor path: a sample packed next to longer ones sees the padded length under proportional attention);
* the refusals by name, outputs untouched;
* the img2img driver with a mask: one engine call, the kept region of the output is the encoded source."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib, models
from lumina_t2x_amd.engine import EngineLimits
from lumina_t2x_amd.transport import masked as MK
from lumina_t2x_amd.transport.mini import ODE
from oracle import synth

import masked_torch as M
from gpu_util import P, lib, stream
from test_gpu_sde import _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
_CACHE = {}


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["hard", "eighths", "soft"])
@pytest.mark.parametrize("mode", [0, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_combine_kernel_equals_the_torch_expressions_word_for_word(dtype, mode, mask_kind):
    n = 4097  # no multiple of the block or of any vector width
    y0, k1, k2, k3, k4 = M.slopes(n, dtype, 21, "cuda")
    _, m, noise, x1 = M.operands(n, dtype, 22, mask_kind, "cuda")
    dt = torch.tensor(0.2371, device="cuda")  # a 0-dim device tensor, as t1 - t0 of the loop: a bf16 state sees it cast to bf16
    dt_arg = float(dt.to(dtype))
    assert dtype == torch.float32 or dt_arg != float(dt)
    step = M.step(mode, y0, k1, k2, k3, k4, dt)
    assert step.dtype == dtype and bool(torch.isfinite(step.float()).all())
    code = _lib.LT_BF16 if dtype == torch.bfloat16 else _lib.LT_F32
    for t in M.T_VALUES:
        t32 = float(np.float32(t))  # the loop holds float(tgrid[i + 1]): an fp32 grid value
        omt = float(np.float32(1.0 - t32))  # 1 - t: double, then fp32
        want = M.blend(step, m, noise, x1, t32)
        assert want.dtype == dtype and bool(torch.isfinite(want.float()).all())
        out = torch.full((n + 64,), 7.0, dtype=dtype, device="cuda")  # the words behind n keep the sentinel
        rc = lib().lt_op_ode_combine_masked(mode, P(y0), P(k1), P(k2), P(k3), P(k4), P(m), P(x1), P(noise), P(out), code, dt_arg, t32, omt, n, stream())
        _lib.check(rc, "lt_op_ode_combine_masked")
        bad = M.bits(out[:n]) != M.bits(want)
        assert not bool(bad.any()), (t, int(bad.sum()), int(bad.nonzero()[0]))
        assert bool((out[n:] == 7.0).all())
        # and torch on this device computes the chain of the documentation
        assert torch.equal(M.bits(want), M.bits(M.chain64(step, m, noise, x1, t32, dtype))), t


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
def _next(golden_dir):
    if "next" not in _CACHE:
        model, z, kw = _model(golden_dir, "next")
        _CACHE["next"] = (model, kw)
    return _CACHE["next"]


def _masks(B, H, W, dtype):
    rect = torch.zeros(H, W)
    rect[3:H - 4, 5:W - 2] = 1.0
    ramp = (torch.arange(W).float() / (W - 1)).expand(H, W).contiguous()
    return {"rect": rect.cuda(), "ramp": ramp.cuda(), "ones": torch.ones(1, 1, H, W, device="cuda"), "zeros": torch.zeros(B, 1, H, W, device="cuda")}


def _grid(name):
    if name == "cut":  # as img2img cuts it: starts at t0 > 0
        o = ODE(9, "midpoint", 4, strength=0.6)
        assert float(o.t[0]) > 0 and len(o.t) == 6
        return "midpoint", o.t
    return name, ODE(5, name, 4).t


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", ["euler", "midpoint", "rk4", "cut"])
def test_engine_trajectory_equals_the_host_loop_state_for_state(golden_dir, case, dtype):
    model, kw = _next(golden_dir)
    method, tgrid = _grid(case)
    stages = {"euler": 1, "midpoint": 2, "rk4": 4}[method]
    cap, cmask = kw["cap_feats"], kw["cap_mask"]
    step_kw = dict(proportional_attn=True, base_seqlen=16)
    g = torch.Generator().manual_seed(4)
    # B = 2 with guidance on the square latent, B = 3 without on the rectangular one
    for B, H, W, guided in ((2, 16, 16, True), (3, 16, 24, False)):
        Bh = B // 2 if guided else B
        x1 = torch.randn(Bh, 4, H, W, generator=g).to("cuda", dtype)
        noise = torch.randn(Bh, 4, H, W, generator=g).to("cuda", dtype)
        t0 = float(tgrid[0])
        z = MK.known(noise, x1, t0)
        if guided:
            z = z.repeat(2, 1, 1, 1)
            cf, cm = cap[:2], cmask[:2]
            host_fn, host_kw = model.forward_with_cfg, dict(cap_feats=cf, cap_mask=cm, cfg_scale=4.0, **step_kw)
            eng_kw = dict(cfg_scale=4.0, **step_kw)
        else:
            cf, cm = torch.cat([cap, cap[:1]]), torch.cat([cmask, cmask[:1]])
            model.forward_with_cfg(z[:2], torch.zeros(2, device="cuda"), cap[:2], cmask[:2], 4.0, **step_kw)  # the flags a plain forward reads
            host_fn, host_kw = model.forward, dict(cap_feats=cf, cap_mask=cm)
            eng_kw = dict(cfg_scale=None)
        o = ODE(5, method, 4)
        o.t = tgrid
        unmasked = o.sample(z, host_fn, **host_kw)  # lt_sample_ode
        nfe = model._engine.last_nfe()
        assert nfe == (len(tgrid) - 1) * stages
        for name, m in _masks(B, H, W, dtype).items():
            got = model.sample_ode_masked(z, tgrid, m, x1, noise, cf, cm, method=method, return_trajectory=True, **eng_kw)
            assert model._engine.last_nfe() == nfe, name
            em, ex, en = MK.expand_operands(z, m, x1, noise)
            want = MK.sample_masked(host_fn, z, tgrid, em, ex, en, method, **host_kw)
            tag = (case, dtype, B, name)
            assert got.shape == want.shape == (len(tgrid),) + tuple(z.shape) and got.dtype == dtype, tag
            assert bool(torch.isfinite(want.float()).all()), tag
            for i in range(len(tgrid)):
                assert torch.equal(got[i], want[i]), tag + (i, int((got[i] != want[i]).sum()))
            final = model.sample_ode_masked(z, tgrid, m, x1, noise, cf, cm, method=method, **eng_kw)
            assert torch.equal(final, got[-1]), tag
            if name == "ones":
                assert torch.equal(got, unmasked), tag
            elif name == "zeros":
                assert torch.equal(M.bits(got[-1]), M.bits(ex)), tag
            else:
                keep = em == 0
                assert torch.equal(got[-1][keep], ex[keep]) and not torch.equal(got[-1], unmasked[-1]), tag
                if name == "rect":  # the generated region is not the unmasked run's either: its surroundings differ
                    assert not torch.equal(got[-1][em == 1], unmasked[-1][em == 1]), tag
        # through the transport front end: the same call, and the host loop with use_engine = False
        m = _masks(B, H, W, dtype)["ramp"]
        via = o.sample(z, host_fn, mask=m, x1=x1, noise=noise, **host_kw)
        assert model._engine.last_nfe() == nfe
        o.use_engine = False
        assert torch.equal(via, o.sample(z, host_fn, mask=m, x1=x1, noise=noise, **host_kw))


def test_a_class_conditional_family_runs_the_same_call(golden_dir):
    model, z, kw = _model(golden_dir, "imagenet")
    z = z.to("cuda", torch.bfloat16)
    g = torch.Generator().manual_seed(9)
    x1, noise = (torch.randn(1, 4, 16, 16, generator=g).to("cuda", torch.bfloat16) for _ in range(2))
    m = _masks(2, 16, 16, torch.bfloat16)["rect"]
    o = ODE(5, "midpoint", 4)
    got = o.sample(z, model.forward_with_cfg, mask=m, x1=x1, noise=noise, **kw)
    assert model._engine.last_nfe() == 8
    o.use_engine = False
    want = o.sample(z, model.forward_with_cfg, mask=m, x1=x1, noise=noise, **kw)
    assert got.shape == (5,) + tuple(z.shape) and bool(torch.isfinite(want.float()).all())
    for i in range(5):
        assert torch.equal(got[i], want[i]), i
    assert torch.equal(got[-1][:, :, m == 0], x1.expand_as(z)[:, :, m == 0])


# ---- packed --------------------------------------------------------------------------------------------------------------------------
def _packed_model(golden_dir):
    if "packed" not in _CACHE:
        g = np.load(os.path.join(golden_dir, "nextdit_tiny_packed_cfg.npz"), allow_pickle=False)
        cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
        m = models.NextDiT(**cfg.ctor_kwargs())
        m.load_state_dict(synth.synth_state_dict(cfg, seed=int(g["seed_w"])), strict=True)
        _CACHE["packed"] = (m.eval().to("cuda", torch.bfloat16), torch.from_numpy(g["cap"]).to("cuda", torch.bfloat16), torch.from_numpy(g["mask"]).cuda())
    return _CACHE["packed"]


@pytest.mark.parametrize("method", ["euler", "midpoint"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_packed_call_equals_the_host_loop_on_the_flat_state(golden_dir, dtype, method):
    model, cap, cmask = _packed_model(golden_dir)
    sizes = [(16, 16), (16, 12), (12, 16)]  # 64, 48, 48 tokens: the longest a multiple of 64 (the one-wave kernel), two shapes of one length
    assert max((h // 2) * (w // 2) for h, w in sizes) % 64 == 0
    g = torch.Generator().manual_seed(6)
    x1s = [torch.randn(4, h, w, generator=g).to("cuda", dtype) for h, w in sizes]
    nzs = [torch.randn(4, h, w, generator=g).to("cuda", dtype) for h, w in sizes]
    tgrid = ODE(5, method, 4).t[1:]  # starts at t0 > 0
    t0 = float(tgrid[0])
    zs = [MK.known(n, x, t0) for n, x in zip(nzs, x1s)]
    zs = zs + [z.clone() for z in zs]
    masks = []
    for k, (h, w) in enumerate(sizes):
        m = torch.zeros(h, w, device="cuda")
        if k == 0:
            m[2:9, 4:13] = 1.0
        elif k == 1:
            m[:] = (torch.arange(w, device="cuda").float() / (w - 1))
        else:
            m[:, : w // 2] = 0.625
        masks.append(m)
    kw = dict(proportional_attn=True, base_seqlen=16)
    got = model.sample_ode_masked_packed(zs, tgrid, masks, x1s, nzs, cap, cmask, 4.0, method=method, return_trajectory=True, **kw)
    stages = {"euler": 1, "midpoint": 2}[method]
    assert model._engine.last_nfe() == (len(tgrid) - 1) * stages
    ems, exs, ens = MK.expand_operands_packed(zs, masks, x1s, nzs)
    shapes, counts = [tuple(z.shape) for z in zs], [z.numel() for z in zs]
    flat = lambda vs: torch.cat([v.reshape(-1) for v in vs])  # noqa: E731

    def model_fn(y, tvec):
        parts = [p.view(s) for p, s in zip(y.split(counts), shapes)]
        return flat(model.forward_with_cfg_packed(parts, tvec, cap, cmask, 4.0, **kw))

    want = MK.sample_masked(model_fn, flat(zs), tgrid, flat(ems), flat(exs), flat(ens), method, batch=len(zs))
    assert bool(torch.isfinite(want.float()).all())
    for b, out in enumerate(got):
        assert tuple(out.shape) == (len(tgrid),) + shapes[b] and out.dtype == dtype
        w = torch.stack([want[i].split(counts)[b].view(shapes[b]) for i in range(len(tgrid))])
        assert torch.equal(out, w), (b, int((out != w).sum()))
        keep = ems[b] == 0
        assert torch.equal(out[-1][keep], exs[b][keep]), b
    final = model.sample_ode_masked_packed(zs, tgrid, masks, x1s, nzs, cap, cmask, 4.0, method=method, **kw)
    assert all(torch.equal(f, o[-1]) for f, o in zip(final, got))
    # mask = 1 everywhere: the unmasked packed sampler's states
    ones = [torch.ones(h, w, device="cuda") for h, w in sizes]
    a = model.sample_ode_masked_packed(zs, tgrid, ones, x1s, nzs, cap, cmask, 4.0, method=method, return_trajectory=True, **kw)
    b = model.sample_ode_packed(zs, tgrid, cap, cmask, 4.0, method=method, return_trajectory=True, **kw)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched(golden_dir):
    model, cap, cmask = _packed_model(golden_dir)
    n = 2 * 4 * 16 * 16
    z = torch.zeros(2, 4, 16, 16, dtype=torch.bfloat16, device="cuda")
    lim = model.engine_limits  # room for a batch of 3, whichever tests ran before: the odd batch must reach its own refusal
    model.engine_limits = EngineLimits(max(lim.max_batch, 6), lim.max_tokens, lim.max_text)
    model.forward_with_cfg(z, torch.full((2,), 0.5, device="cuda"), cap[:2], cmask[:2], 4.0)  # engine, weights, a prompt of 2 rows
    eng, L = model._engine, lib()
    out = torch.full((8 * n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    buf = torch.zeros(4 * n, dtype=torch.bfloat16, device="cuda")
    grid = (C.c_float * 3)(0.0, 0.5, 1.0)
    null = C.c_void_p(0)

    def tensor(*, mask=P(buf), x1=P(buf), noise=P(buf), method=0, ng=3, batch=2, use_cfg=1):
        a = eng._step_args(z, 4.0, 1.0, 1.0, None, False)
        a.batch = batch
        return L.lt_sample_ode_masked(eng.handle, P(z), mask, x1, noise, P(out), P(out[4 * n:]), grid, ng, method, use_cfg, 1, C.byref(a), stream())

    def packed(*, mask=P(buf), x1=P(buf), noise=P(buf), method=0, ng=3, batch=2, use_cfg=1):
        a = eng._step_args(z.view(1, 1, 1, -1), 4.0, 1.0, 1.0, None, False)
        a.batch, a.latent_h, a.latent_w = batch, 0, 0
        hw = (C.c_int32 * (2 * batch))(*([16, 16] * batch))
        return L.lt_sample_ode_masked_packed(eng.handle, P(z), hw, mask, x1, noise, P(out), P(out[4 * n:]), grid, ng, method, use_cfg, 1, C.byref(a),
                                             stream())

    def refused(rc, *words):
        msg = L.lt_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), msg

    for call, who in ((tensor, "lt_sample_ode_masked:"), (packed, "lt_sample_ode_masked_packed:")):
        refused(call(mask=null), who, "null mask, source or noise")
        refused(call(x1=null), who, "null mask, source or noise")
        refused(call(noise=null), who, "null mask, source or noise")
        refused(call(method=7), who, "unknown method")
        refused(call(method=-1), who, "unknown method")
        refused(call(ng=1), who, "2 grid points")
        refused(call(batch=3), "even batch")
    refused(tensor(batch=0), "batch 0 outside")
    with pytest.raises(_lib.LuminaLibError, match="not in"):
        eng.sample_ode_masked(z, [0.0, 1.0], z, z, z, "heun2", use_cfg=True)
    with pytest.raises(_lib.LuminaLibError, match="layout and dtype of the state"):
        eng.sample_ode_masked(z, [0.0, 1.0], z[:1], z, z, "euler", use_cfg=True)
    with pytest.raises(_lib.LuminaLibError, match="layout and dtype of the state"):
        eng.sample_ode_masked(z, [0.0, 1.0], z, z.float(), z, "euler", use_cfg=True)
    # ... and the same arguments untouched are served
    assert tensor() == 0 and packed() == 0, L.lt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:3 * n].float()).all()) and eng.last_nfe() == 2


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_img2img_driver_with_a_mask_keeps_the_source_and_is_one_engine_call(golden_dir, tmp_path):
    import argparse

    from safetensors.torch import save_file

    from lumina_t2x_amd import sample_img2img as S

    g = np.load(os.path.join(golden_dir, "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    ck = tmp_path / "ckpt"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "consolidated_ema.00-of-01.safetensors"))
    torch.save(argparse.Namespace(model="NextDiT_tiny_masked_test", qk_norm=cfg.qk_norm, image_size=256, vae="sdxl"), str(ck / "model_args.pth"))
    built = []

    def ctor(**kw):
        built.append(models.NextDiT(**{**cfg.ctor_kwargs(), **kw}))
        return built[-1]

    models.__dict__["NextDiT_tiny_masked_test"] = ctor
    (tmp_path / "prompts.txt").write_text("a red cube\n")
    gen = torch.Generator().manual_seed(5)
    table = {c: torch.randn(16, cfg.cap_feat_dim, generator=gen) for c in ("a red cube", "")}
    image = torch.rand(3, 128, 128, generator=gen).mul(2).sub(1).cuda()
    pix = torch.zeros(128, 128)
    pix[32:96, 40:100] = 1.0  # pixel columns 96..99 are half of latent column 12: a soft edge

    def encode(caps):
        feats = torch.stack([table[c] for c in caps]).to("cuda", torch.bfloat16)
        mask = torch.ones(len(caps), 16, dtype=torch.int64, device="cuda")
        mask[-1, 8:] = 0
        return feats, mask

    def vae_encode(img):  # a stand-in "VAE": 8 x 8 average pooling to 4 channels
        return torch.nn.functional.avg_pool2d(torch.cat([img, img[:, :1]], dim=1), 8)

    decoded = []

    def decode(lat):
        decoded.append(lat.clone())
        return torch.sigmoid(lat[:, :3].float())

    argv = ["--ckpt", str(ck), "--image", "unused.png", "--caption_path", str(tmp_path / "prompts.txt"), "--resolution", "256:128x128",
            "--num_sampling_steps", "9", "--solver", "midpoint", "--strength", "0.6", "--time_shifting_factor", "4", "--seed", "13"]
    try:
        S.run(S.build_parser().parse_args(argv + ["--image_save_path", str(tmp_path / "a")]), encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim,
              vae_encode_fn=vae_encode, decode_fn=decode, image=image, mask=pix)
        nfe = built[-1]._engine.last_nfe()
        S.run(S.build_parser().parse_args(argv + ["--image_save_path", str(tmp_path / "b")]), encode_fn=encode, cap_feat_dim=cfg.cap_feat_dim,
              vae_encode_fn=vae_encode, decode_fn=decode, image=image)
    finally:
        del models.__dict__["NextDiT_tiny_masked_test"]
    ode = ODE(9, "midpoint", 4.0, strength=0.6)
    assert nfe == 2 * (len(ode.t) - 1)  # every evaluation of the run lies in ONE whole-trajectory call
    x1 = vae_encode(image[None]).mul(0.13025).to(torch.bfloat16)
    m = S.latent_mask(pix, 16, 16)[0, 0].cuda()
    assert 0 < int((m == 0).sum()) < 256 and bool(((m > 0) & (m < 1)).any())
    # the decoder sees latent / factor: where the mask says keep that is the encoded source, word for word; plain img2img moves it
    assert torch.equal(decoded[0][:, :, m == 0], (x1 / 0.13025)[:, :, m == 0])
    assert not torch.equal(decoded[1][:, :, m == 0], (x1 / 0.13025)[:, :, m == 0])
    assert not torch.equal(decoded[0][:, :, m == 1], decoded[1][:, :, m == 1])
    # the whole latent is the hand-made call
    torch.random.manual_seed(13)
    noise = torch.randn([1, 4, 16, 16], device="cuda").to(torch.bfloat16)
    z = MK.known(noise, x1, float(ode.t[0])).repeat(2, 1, 1, 1)
    feats, cmask = encode(["a red cube", ""])
    model = built[0]
    want = model.sample_ode_masked(z, ode.t, S.latent_mask(pix, 16, 16).cuda(), x1, noise, feats, cmask, 4.0, method="midpoint",
                                   proportional_attn=True, base_seqlen=256)[:1]
    assert torch.equal(decoded[0], want / 0.13025)
