"""Text-to-image sampling driver on the MI355X engine - command-line compatible with the reference's
``lumina_next_t2i/sample.py`` (argument names and defaults :267-330, output layout ``<image_save_path>/images/*.png`` +
``data.json`` :144-260) for the step either side of the hot path:

    caption --[text encoder, hidden_states[-2] (:47-51)]--> cap_feats, cap_mask
    z ~ N(0, I) [1,4,h/8,w/8] repeated for cond + uncond (:201-203) --[Sampler.sample_ode on the engine]--> latent
    latent / vae_scale --[VAE decoder (:237-240)]--> png

What is ours: one process per GPU under ``python -m torch.distributed.run`` (RANK / WORLD_SIZE from the environment, captions
sharded round-robin, no collective on the data path) instead of mp.spawn + fairscale model-parallel groups; the DiT runs on
the HIP engine behind ``models.NextDiT``.  What stays third-party, exactly as in the reference: the text encoder
(``transformers.AutoModel``) and the VAE (``diffusers.AutoencoderKL``).  Both are loaded from LOCAL paths (no network here);
without ``diffusers`` the driver writes the final latents as ``.pt`` files instead of pngs and says so.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m lumina_t2x_amd.sample \\
        --ckpt /ckpts/Lumina-Next-SFT --text_encoder /ckpts/gemma-2b --vae /ckpts/sdxl-vae \\
        --caption_path prompts.txt --resolution 1024:1024x1024 --num_sampling_steps 30 --sampling-method midpoint \\
        --time_shifting_factor 4
"""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import Callable, List, Optional, Tuple

import torch

from . import models
from .transport import Sampler, create_transport

VAE_SCALE = {"sdxl": 0.13025}  # everything else 0.18215 (reference sample.py:236)


def load_train_args(ckpt_dir: str):
    """``model_args.pth`` is the pickled argparse.Namespace of the training run (reference sample.py:98)."""
    return torch.load(os.path.join(ckpt_dir, "model_args.pth"), map_location="cpu", weights_only=False)


def load_checkpoint(ckpt_dir: str, ema: bool) -> dict:
    """consolidated{_ema}.00-of-01.{safetensors,pth} (single model-parallel rank: the engine holds whole weights)."""
    stem = os.path.join(ckpt_dir, f"consolidated{'_ema' if ema else ''}.00-of-01")
    if os.path.exists(stem + ".safetensors"):
        from safetensors.torch import load_file
        return load_file(stem + ".safetensors", device="cpu")
    if os.path.exists(stem + ".pth"):
        return torch.load(stem + ".pth", map_location="cpu", weights_only=True)
    import glob
    shards = sorted(glob.glob(os.path.join(ckpt_dir, f"consolidated{'_ema' if ema else ''}.*-of-*.*")))
    if shards:
        # train.py:625-634 writes one file per model-parallel rank.  They are not a split of ONE model: with qk_norm the reference builds
        # q_norm / k_norm as nn.LayerNorm(n_LOCAL_heads * head_dim) (models/model.py:211-215) - each rank normalises over ITS heads only, so an
        # MP = k checkpoint computes k grouped LayerNorms where the MP = 1 model (every released checkpoint) computes one over the full width.
        # Concatenating the Column / RowParallelLinear shards would load, and sample something else.
        raise FileNotFoundError(f"{ckpt_dir} holds model-parallel shards ({', '.join(os.path.basename(f) for f in shards)}); this engine loads "
                                "model-parallel size 1 only: with qk_norm the reference's q / k LayerNorms span the LOCAL heads of each rank "
                                "(models/model.py:211-215), so an MP > 1 checkpoint is a different function from the concatenation of its shards")
    raise FileNotFoundError(f"{stem}.safetensors / .pth not found")


def make_text_encoder(path: str, dtype, device, add_eos: bool = True) -> Tuple[Callable[[List[str]], Tuple[torch.Tensor, torch.Tensor]], int]:
    """(encode(captions) -> (feats [n, T, C], mask [n, T]), C) with the reference's tokenizer settings (sample.py:34-51;
    ``add_eos=False`` is the ``lumina_next`` CLI's tokenizer, utils/cli.py:121)."""
    from transformers import AutoModel, AutoTokenizer
    tok = AutoTokenizer.from_pretrained(path, add_eos=True) if add_eos else AutoTokenizer.from_pretrained(path)
    tok.padding_side = "right"
    enc = AutoModel.from_pretrained(path, torch_dtype=dtype).to(device).eval()

    @torch.no_grad()
    def encode(captions):
        ti = tok(captions, padding=True, pad_to_multiple_of=8, max_length=256, truncation=True, return_tensors="pt")
        out = enc(input_ids=ti.input_ids.to(device), attention_mask=ti.attention_mask.to(device), output_hidden_states=True)
        return out.hidden_states[-2], ti.attention_mask.to(device)

    return encode, enc.config.hidden_size


def make_vae_decoder(path: Optional[str], device) -> Optional[Callable[[torch.Tensor], torch.Tensor]]:
    """latent (already divided by the scale factor) -> image in [0, 1]; None when diffusers / the weights are unavailable."""
    if not path:
        return None
    try:
        from diffusers.models import AutoencoderKL
    except ImportError:
        return None
    vae = AutoencoderKL.from_pretrained(path, torch_dtype=torch.float32).to(device).eval()

    @torch.no_grad()
    def decode(lat):
        return ((vae.decode(lat.float()).sample + 1.0) / 2.0).clamp_(0.0, 1.0)

    return decode


def parse_resolution(spec: str) -> Tuple[int, int, int]:
    """'1024:1024x1024' -> (category, w, h) (reference sample.py:193-199)."""
    cat, wh = spec.split(":")
    w, h = wh.split("x")
    return int(cat), int(w), int(h)


def save_png(img: torch.Tensor, path: str) -> None:
    """[3, H, W] in [0, 1] -> 8-bit png (PIL if present, else a minimal zlib writer: no torchvision here)."""
    arr = (img.float().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
    try:
        from PIL import Image
        Image.fromarray(arr).save(path)
        return
    except ImportError:
        pass
    import struct
    import zlib
    h, w, _ = arr.shape
    raw = b"".join(b"\x00" + arr[r].tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def tile_windows(args, canvas_hw, patch_size: int = 2):
    """``--tile H W [--tile_stride SH SW] [--tile_weights KIND]`` (pixels) on a canvas latent of ``canvas_hw`` -> ``((offsets, (win_h, win_w)),
    weights)`` in latent pixels.  The driver draws its latent width first (``[1, 4, w / 8, h / 8]``, as the reference does), so W goes with the
    latent's first spatial axis and H with its second, like the resolution; a tile larger than the canvas is clamped to it; the default
    stride is half the tile."""
    from .transport.tiled import window_grid, window_weights
    th_px, tw_px = args.tile
    stride = getattr(args, "tile_stride", None) or (th_px // 2, tw_px // 2)
    unit = 8 * patch_size
    for name, v in (("--tile", (th_px, tw_px)), ("--tile_stride", tuple(stride))):
        if any(int(x) < unit or int(x) % unit for x in v):
            raise SystemExit(f"{name} {v[0]} {v[1]}: sizes are pixels, positive multiples of {unit} (8 per latent pixel x the patch size {patch_size})")
    win = (min(tw_px // 8, canvas_hw[0]), min(th_px // 8, canvas_hw[1]))
    st = (min(stride[1] // 8, win[0]), min(stride[0] // 8, win[1]))
    try:
        offsets = window_grid(canvas_hw[0], canvas_hw[1], win[0], win[1], st[0], st[1], patch_size)
    except ValueError as exc:
        raise SystemExit(f"--tile: {exc}") from None
    return (offsets, win), window_weights(win[0], win[1], getattr(args, "tile_weights", "uniform") or "uniform")


def compose_plan(args, tgrid):
    """``--compose_prompts P1 .. PK --compose_weights W1 .. WK [--compose_interval K LO HI]...`` -> ``(prompts, table)`` with the weight table
    of ``transport.guidance.compose_table`` (prompt K, counted from 1, weighs 0 outside its interval); ``None`` without ``--compose_prompts``"""
    prompts = getattr(args, "compose_prompts", None)
    weights, intervals = getattr(args, "compose_weights", None), getattr(args, "compose_interval", None) or []
    if not prompts:
        if weights or intervals:
            raise SystemExit("--compose_weights / --compose_interval belong to --compose_prompts")
        return None
    from .transport import guidance
    if not weights or len(weights) != len(prompts):
        raise SystemExit(f"--compose_prompts names {len(prompts)} prompts: --compose_weights needs as many weights, got {len(weights or [])}")
    if len(prompts) > guidance.COMPOSE_MAX:
        raise SystemExit(f"--compose_prompts: {len(prompts)} prompts, at most {guidance.COMPOSE_MAX} are served")
    per = [None] * len(prompts)
    for k, lo, hi in intervals:
        if k != int(k) or not 1 <= int(k) <= len(prompts):
            raise SystemExit(f"--compose_interval {k:g} {lo:g} {hi:g}: the prompt is counted from 1 to {len(prompts)}")
        per[int(k) - 1] = (lo, hi)
    try:
        return list(prompts), guidance.compose_table(tgrid, args.sampling_method, [float(w) for w in weights], per)
    except ValueError as exc:
        raise SystemExit(f"--compose_prompts: {exc}") from None


def run(args, *, encode_fn=None, cap_feat_dim=None, decode_fn=None, model=None) -> List[dict]:
    """Sample every (resolution, caption) pair of this rank's shard.  ``encode_fn`` / ``decode_fn`` / ``model`` can be injected
    (tests, or a caller that already holds the encoder / VAE); otherwise they are built from the command-line paths."""
    torch.set_grad_enabled(False)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[args.precision]
    train_args = load_train_args(args.ckpt)
    if encode_fn is None:
        encode_fn, cap_feat_dim = make_text_encoder(args.text_encoder, dtype, device)
    if model is None:
        model = models.__dict__[train_args.model](qk_norm=train_args.qk_norm, cap_feat_dim=cap_feat_dim)
        model.eval().to(device, dtype=dtype)
        if not args.debug:
            model.load_state_dict(load_checkpoint(args.ckpt, args.ema), strict=True)
    if decode_fn is None:
        decode_fn = make_vae_decoder(args.vae, device)
        if decode_fn is None and rank == 0:
            print("[sample] no VAE decoder (diffusers or --vae missing): writing final latents as .pt", flush=True)
    out_dir = args.image_save_path
    os.makedirs(os.path.join(out_dir, "images"), exist_ok=True)
    with open(args.caption_path, "r", encoding="utf-8") as f:
        captions = [ln.strip() for ln in f if ln.strip()]
    vae_name = getattr(train_args, "vae", "sdxl")
    factor = VAE_SCALE.get(vae_name, 0.18215)
    info: List[dict] = []
    jobs = [(res, i, c) for res in args.resolution for i, c in enumerate(captions)]
    for j, (res, idx, caption) in enumerate(jobs):
        if j % world != rank:
            continue
        cat, w, h = parse_resolution(res)
        transport = create_transport(args.path_type, args.prediction, args.loss_weight, args.train_eps, args.sample_eps)
        sample_fn = Sampler(transport).sample_ode(sampling_method=args.sampling_method, num_steps=args.num_sampling_steps,
                                                  atol=args.atol, rtol=args.rtol, reverse=args.reverse,
                                                  time_shifting_factor=args.time_shifting_factor)
        if int(args.seed) != 0:
            torch.manual_seed(int(args.seed))
        # note: the reference draws [1, 4, w/8, h/8] (sample.py:201-202), i.e. width first - kept
        z = torch.randn([1, 4, w // 8, h // 8], device=device).to(dtype).repeat(2, 1, 1, 1)
        cap_feats, cap_mask = encode_fn([caption, ""])
        kw = dict(cap_feats=cap_feats, cap_mask=cap_mask.to(cap_feats.device), cfg_scale=args.cfg_scale,
                  proportional_attn=bool(args.proportional_attn),
                  base_seqlen=(train_args.image_size // 16) ** 2 if args.proportional_attn else None)
        if cat > 1024 and args.scaling_method == "Time-aware":
            kw.update(scale_factor=math.sqrt(w * h / train_args.image_size ** 2), scale_watershed=args.scaling_watershed)
        else:
            kw.update(scale_factor=1.0, scale_watershed=1.0)
        tile = getattr(args, "tile", None)
        if tile:  # the model sees windows of the tile's size, not the canvas
            kw.update(scale_factor=1.0, scale_watershed=1.0)
            if tile[0] * tile[1] > train_args.image_size ** 2 and args.scaling_method == "Time-aware":
                kw.update(scale_factor=math.sqrt(tile[0] * tile[1] / train_args.image_size ** 2), scale_watershed=args.scaling_watershed)
        table = guidance_table(args, sample_fn.__self__.t)
        rule = guidance_rule(args)
        reuse = guidance_reuse(args, sample_fn.__self__.t, table)
        pag = guidance_pag(args, sample_fn.__self__.t)
        seg = guidance_seg(args, sample_fn.__self__.t)
        slg = None if (pag is not None or seg is not None) else guidance_slg(args, sample_fn.__self__.t)
        tea = step_cache(args)
        proj = guidance_project(args)
        comp = compose_plan(args, sample_fn.__self__.t)
        if seg is not None:  # a third evaluation of the prompt row with some blocks' queries blurred; with the scale table and --slg_layers alone
            if comp or tile or proj or tea or pag is not None:
                raise SystemExit("--seg_layers is not served together with --compose_prompts, --tile, --apg_* / --cfg_zero_star, --teacache or --pag_*")
            if table is None:
                from .transport import guidance
                table = guidance.cfg_table(sample_fn.__self__.t, args.sampling_method, args.cfg_scale)
            latent = sample_fn(z, model.forward_with_cfg, cfg_table=table, seg_table=seg, seg_layers=list(args.seg_layers),
                               seg_sigma=float(args.seg_sigma), slg_layers=list(getattr(args, "slg_layers", None) or []), **kw)[-1][:1]
        elif comp:  # composed guidance: the K prompts of --compose_prompts stand in for the caption, the negative prompt is the base row
            if tile or table is not None or rule or reuse is not None or pag is not None or slg is not None or tea or proj:
                raise SystemExit("--compose_prompts is not served together with --tile, --cfg_interval / --cfg_schedule, --cfg_rescale / "
                                 "--cfg_norm_limit, --cfg_reuse*, --slg_*, --pag_*, --teacache, --apg_* or --cfg_zero_star")
            feats, cmask = encode_fn(comp[0] + [""])
            ckw = dict(kw, cap_feats=feats, cap_mask=cmask.to(feats.device))
            latent = sample_fn(z[:1], model.forward_with_cfg, compose=comp[1], **ckw)[-1][:1]
        elif tile:  # MultiDiffusion: ONE canvas latent, every stage the model on overlapping windows of it, their predictions fused
            if table is not None or rule or reuse is not None or pag is not None or slg is not None or tea or proj:
                raise SystemExit("--tile is not served together with --cfg_interval / --cfg_schedule, --cfg_rescale / --cfg_norm_limit, --cfg_reuse*, "
                                 "--slg_*, --pag_*, --teacache, --apg_* or --cfg_zero_star")
            windows, weights = tile_windows(args, tuple(z.shape[2:]), getattr(model, "patch_size", 2))
            latent = sample_fn(z[:1], model.forward_with_cfg, windows=windows, window_weights=weights, **kw)[-1][:1]
        elif proj:  # APG / CFG-Zero*: the guided stages built on inner products of the two rows; combines with the scale table alone
            if rule or reuse is not None or pag is not None or slg is not None or tea:
                raise SystemExit("--apg_* / --cfg_zero_star are not served together with --cfg_rescale / --cfg_norm_limit, --cfg_reuse*, "
                                 "--slg_*, --pag_* or --teacache")
            latent = sample_fn(z, model.forward_with_cfg, cfg_table=table, **proj, **kw)[-1][:1]
        elif pag is not None:  # a third evaluation of the prompt row with some blocks' self-attention map replaced by the identity
            if tea:
                raise SystemExit("--pag_layers is not served together with --teacache")
            if table is None:
                from .transport import guidance
                table = guidance.cfg_table(sample_fn.__self__.t, args.sampling_method, args.cfg_scale)
            latent = sample_fn(z, model.forward_with_cfg, cfg_table=table, pag_table=pag, pag_layers=list(args.pag_layers),
                               slg_layers=list(getattr(args, "slg_layers", None) or []), **kw)[-1][:1]
        elif tea:  # evaluations whose first-block input barely moved leave the block stack out (the TeaCache rule)
            latent = sample_fn(z, model.forward_with_cfg, **tea, **kw)[-1][:1]
        elif slg is not None:  # stages that also evaluate the prompt row with some blocks left out and push away from it
            if table is None:
                from .transport import guidance
                table = guidance.cfg_table(sample_fn.__self__.t, args.sampling_method, args.cfg_scale)
            latent = sample_fn(z, model.forward_with_cfg, cfg_table=table, slg_table=slg, slg_layers=list(args.slg_layers), **kw)[-1][:1]
        elif reuse is not None:  # guided stages that reuse the last refresh stage's cond - uncond difference at half the rows
            latent = sample_fn(z, model.forward_with_cfg, cfg_table=table, cfg_reuse=reuse, **kw)[-1][:1]
        elif table is None and not rule:
            latent = sample_fn(z, model.forward_with_cfg, **kw)[-1][:1]
        elif not rule:  # a scale per stage; stages at scale 1 evaluate the cond row alone (transport/guidance.py)
            latent = sample_fn(z, model.forward_with_cfg, cfg_table=table, **kw)[-1][:1]
        else:  # ... and the guided stages rescaled / norm-limited per sample (without a table: --cfg_scale at every stage)
            latent = sample_fn(z, model.forward_with_cfg, cfg_table=table, **rule, **kw)[-1][:1]
        stem = os.path.join(out_dir, "images", f"{args.sampling_method}_{args.num_sampling_steps}_{idx}_{res.split(':')[-1]}")
        if decode_fn is not None:
            save_png(decode_fn(latent / factor)[0], stem + ".png")
            url = stem + ".png"
        else:
            torch.save(latent.cpu(), stem + ".pt")
            url = stem + ".pt"
        info.append({"caption": caption, "image_url": url, "resolution": f"res: {res.split(':')[-1]}\ntime_shift: {args.time_shifting_factor}",
                     "sampling_method": args.sampling_method, "num_sampling_steps": args.num_sampling_steps})
    with open(os.path.join(out_dir, f"data.rank{rank}.json" if world > 1 else "data.json"), "w") as f:
        json.dump(info, f)
    return info


def guidance_table(args, tgrid):
    """``--cfg_interval`` / ``--cfg_schedule`` as the scale table of ``transport.guidance.cfg_table``; None: one scale for every stage (the
    sampler's plain path)"""
    interval, kind = getattr(args, "cfg_interval", None), getattr(args, "cfg_schedule", "constant")
    if interval is None and kind == "constant":
        return None
    from .transport import guidance
    t0, t1 = float(tgrid[0]), float(tgrid[-1])
    schedule = {"constant": None, "linear": guidance.linear_schedule(args.cfg_scale, t0, t1),
                "cosine": guidance.cosine_schedule(args.cfg_scale, t0, t1)}[kind]
    return guidance.cfg_table(tgrid, args.sampling_method, args.cfg_scale, interval=interval, schedule=schedule)


def guidance_rule(args) -> dict:
    """``--cfg_rescale`` / ``--cfg_norm_limit`` as the sampler's keyword arguments; empty at the defaults: no rule, the call it was"""
    rescale, limit = float(getattr(args, "cfg_rescale", 0.0)), getattr(args, "cfg_norm_limit", None)
    limit = math.inf if limit is None else float(limit)
    if rescale == 0.0 and limit == math.inf:
        return {}
    from .transport import guidance
    rescale, limit = guidance.check_rule(rescale, limit)
    return dict(cfg_rescale=rescale, cfg_norm_limit=limit)


def guidance_project(args) -> dict:
    """``--apg_eta`` / ``--apg_momentum`` / ``--apg_norm_threshold`` or ``--cfg_zero_star`` / ``--cfg_zero_init K`` as the sampler's keyword
    arguments; empty at the defaults: the call it was.  The two forms are exclusive, and built for euler / midpoint / rk4."""
    eta, beta, r = getattr(args, "apg_eta", None), getattr(args, "apg_momentum", None), getattr(args, "apg_norm_threshold", None)
    zero, K = bool(getattr(args, "cfg_zero_star", False)), int(getattr(args, "cfg_zero_init", 0) or 0)
    apg = None
    if eta is not None or beta is not None or r is not None:
        apg = dict(eta=1.0 if eta is None else eta, momentum=0.0 if beta is None else beta, norm_threshold=math.inf if r is None else r)
    if apg is None and not zero and K == 0:
        return {}
    from .transport import guidance
    try:
        form, eta, beta, r, K = guidance.check_project(apg, zero, K)
        guidance.refuse_with_project(form, args.sampling_method)
    except ValueError as exc:
        raise SystemExit(f"--apg_* / --cfg_zero_*: {exc}") from None
    if form == "apg":
        return dict(cfg_apg=dict(eta=eta, momentum=beta, norm_threshold=r))
    return dict(cfg_zero_star=True, cfg_zero_init=K)


def guidance_reuse(args, tgrid, table):
    """``--cfg_reuse K`` / ``--cfg_reuse_per_step`` as the flag table of ``transport.guidance.cfg_reuse_table`` over the scale table (None: one
    scale for every stage); None at the defaults: no reuse, the call it was.  Refused together with ``--cfg_rescale`` / ``--cfg_norm_limit``."""
    every, per_step = int(getattr(args, "cfg_reuse", 0) or 0), bool(getattr(args, "cfg_reuse_per_step", False))
    if every == 0 and not per_step:
        return None
    if guidance_rule(args):
        raise SystemExit("--cfg_reuse / --cfg_reuse_per_step are not served together with --cfg_rescale / --cfg_norm_limit: the rule's sums "
                         "need the prompt and the negative row of every guided stage")
    if every < 0 or every == 1:
        raise SystemExit(f"--cfg_reuse {every}: K >= 2 refreshes the guidance difference on every K-th guided stage (0: off)")
    from .transport import guidance
    if table is None:
        table = guidance.cfg_table(tgrid, args.sampling_method, args.cfg_scale)
    return guidance.cfg_reuse_table(tgrid, args.sampling_method, table, every=max(every, 2), per_step=per_step)


def guidance_slg(args, tgrid):
    """``--slg_layers`` / ``--slg_scale`` / ``--slg_interval`` as the table of ``transport.guidance.slg_table``; None at the defaults (no layers,
    or scale 0): the call it was.  Refused by name together with ``--cfg_rescale`` / ``--cfg_norm_limit``, ``--cfg_reuse*`` and a sampling
    method that is not euler / midpoint / rk4."""
    layers, scale = list(getattr(args, "slg_layers", None) or []), float(getattr(args, "slg_scale", 0.0) or 0.0)
    interval = getattr(args, "slg_interval", None)
    if not layers and scale == 0.0 and interval is None:
        return None
    if not layers:
        raise SystemExit("--slg_scale / --slg_interval need --slg_layers: the blocks the skip evaluation leaves out")
    if guidance_rule(args):
        raise SystemExit("--slg_layers is not served together with --cfg_rescale / --cfg_norm_limit")
    if int(getattr(args, "cfg_reuse", 0) or 0) != 0 or bool(getattr(args, "cfg_reuse_per_step", False)):
        raise SystemExit("--slg_layers is not served together with --cfg_reuse / --cfg_reuse_per_step")
    from .transport import guidance
    if args.sampling_method not in guidance.FIXED_GRID_METHODS:
        raise SystemExit(f"--slg_layers is built for the sampling methods {', '.join(guidance.FIXED_GRID_METHODS)}, not '{args.sampling_method}'")
    try:
        guidance.check_slg_layers(layers)
        if scale == 0.0:
            return None
        return guidance.slg_table(tgrid, args.sampling_method, scale, interval=interval)
    except ValueError as exc:
        raise SystemExit(f"--slg_*: {exc}") from None


def guidance_seg(args, tgrid):
    """``--seg_layers`` / ``--seg_scale`` / ``--seg_sigma`` / ``--seg_interval`` as the table of ``transport.guidance.seg_table``; None at the
    defaults (no layers, or scale 0): the call it was.  ``--slg_layers`` beside it joins the same third evaluation under this one table.  Refused
    by name with what ``--pag_*`` is refused with, and with ``--pag_*``."""
    layers, scale = list(getattr(args, "seg_layers", None) or []), float(getattr(args, "seg_scale", 0.0) or 0.0)
    interval, sigma = getattr(args, "seg_interval", None), getattr(args, "seg_sigma", None)
    if not layers and scale == 0.0 and interval is None and sigma is None:
        return None
    if not layers:
        raise SystemExit("--seg_scale / --seg_sigma / --seg_interval need --seg_layers: the blocks whose queries the third evaluation blurs")
    if getattr(args, "pag_layers", None) or float(getattr(args, "pag_scale", 0.0) or 0.0) != 0.0 or getattr(args, "pag_interval", None) is not None:
        raise SystemExit("--seg_layers together with --pag_* is not served: one third evaluation, and no block is blurred and perturbed")
    if float(getattr(args, "slg_scale", 0.0) or 0.0) != 0.0 or getattr(args, "slg_interval", None) is not None:
        raise SystemExit("--seg_layers together with --slg_scale / --slg_interval is not served: one third evaluation, one scale table "
                         "(--slg_layers beside --seg_layers joins it under --seg_scale)")
    if guidance_rule(args):
        raise SystemExit("--seg_layers is not served together with --cfg_rescale / --cfg_norm_limit")
    if int(getattr(args, "cfg_reuse", 0) or 0) != 0 or bool(getattr(args, "cfg_reuse_per_step", False)):
        raise SystemExit("--seg_layers is not served together with --cfg_reuse / --cfg_reuse_per_step")
    from .transport import guidance
    if args.sampling_method not in guidance.FIXED_GRID_METHODS:
        raise SystemExit(f"--seg_layers is built for the sampling methods {', '.join(guidance.FIXED_GRID_METHODS)}, not '{args.sampling_method}'")
    if sigma is None:
        raise SystemExit("--seg_layers needs --seg_sigma: the width of the blur in tokens (> 0; inf: the mean query)")
    try:
        guidance.check_seg_layers(layers, list(getattr(args, "slg_layers", None) or []))
        guidance.seg_taps(sigma)
        if scale == 0.0:
            return None
        return guidance.seg_table(tgrid, args.sampling_method, scale, interval=interval)
    except ValueError as exc:
        raise SystemExit(f"--seg_*: {exc}") from None


def guidance_pag(args, tgrid):
    """``--pag_layers`` / ``--pag_scale`` / ``--pag_interval`` as the table of ``transport.guidance.pag_table``; None at the defaults (no layers,
    or scale 0): the call it was.  ``--slg_layers`` beside it joins the same third evaluation (those blocks are left out) under this one table;
    a second table (``--slg_scale`` / ``--slg_interval``) is refused by name, as are ``--cfg_rescale`` / ``--cfg_norm_limit``, ``--cfg_reuse*``
    and a sampling method that is not euler / midpoint / rk4."""
    layers, scale = list(getattr(args, "pag_layers", None) or []), float(getattr(args, "pag_scale", 0.0) or 0.0)
    interval = getattr(args, "pag_interval", None)
    if not layers and scale == 0.0 and interval is None:
        return None
    if not layers:
        raise SystemExit("--pag_scale / --pag_interval need --pag_layers: the blocks the third evaluation perturbs")
    if float(getattr(args, "slg_scale", 0.0) or 0.0) != 0.0 or getattr(args, "slg_interval", None) is not None:
        raise SystemExit("--pag_layers together with --slg_scale / --slg_interval is not served: one third evaluation, one scale table "
                         "(--slg_layers beside --pag_layers joins it under --pag_scale)")
    if guidance_rule(args):
        raise SystemExit("--pag_layers is not served together with --cfg_rescale / --cfg_norm_limit")
    if int(getattr(args, "cfg_reuse", 0) or 0) != 0 or bool(getattr(args, "cfg_reuse_per_step", False)):
        raise SystemExit("--pag_layers is not served together with --cfg_reuse / --cfg_reuse_per_step")
    from .transport import guidance
    if args.sampling_method not in guidance.FIXED_GRID_METHODS:
        raise SystemExit(f"--pag_layers is built for the sampling methods {', '.join(guidance.FIXED_GRID_METHODS)}, not '{args.sampling_method}'")
    try:
        guidance.check_pag_layers(layers, list(getattr(args, "slg_layers", None) or []))
        if scale == 0.0:
            return None
        return guidance.pag_table(tgrid, args.sampling_method, scale, interval=interval)
    except ValueError as exc:
        raise SystemExit(f"--pag_*: {exc}") from None


def step_cache(args) -> dict:
    """``--teacache THR`` / ``--teacache_coefficients`` as the sampler's keyword arguments; empty when off: the call it was.  Refused by name
    together with the guidance options, the multistep and adaptive solvers (combining them is later work)."""
    thr, coef = getattr(args, "teacache", None), getattr(args, "teacache_coefficients", None)
    if thr is None:
        if coef is not None:
            raise SystemExit("--teacache_coefficients needs --teacache THR")
        return {}
    from .transport import cache
    rule = float(getattr(args, "cfg_rescale", 0.0) or 0.0), getattr(args, "cfg_norm_limit", None)
    try:
        cache.refuse_with_teacache(args.sampling_method, cfg_interval=getattr(args, "cfg_interval", None),
                                   cfg_schedule=None if getattr(args, "cfg_schedule", "constant") == "constant" else args.cfg_schedule,
                                   cfg_rescale=rule[0], cfg_norm_limit=rule[1],
                                   cfg_reuse=int(getattr(args, "cfg_reuse", 0) or 0) or bool(getattr(args, "cfg_reuse_per_step", False)),
                                   slg=getattr(args, "slg_layers", None) or float(getattr(args, "slg_scale", 0.0) or 0.0)
                                   or getattr(args, "slg_interval", None))
        thr, coef = cache.check_cache_args(thr, cache.IDENTITY if coef is None else coef)
    except ValueError as exc:
        raise SystemExit(f"--teacache: {exc}") from None
    return dict(teacache=thr, teacache_coefficients=coef)


def build_parser() -> argparse.ArgumentParser:
    def none_or_str(v):
        return None if v == "None" else v

    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--cfg_scale", type=float, default=4.0)
    p.add_argument("--cfg_interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="guide only the stages with LO <= t < HI (t = 0 noise, 1 data); the others evaluate the prompt row alone")
    p.add_argument("--cfg_schedule", type=str, default="constant", choices=["constant", "linear", "cosine"],
                   help="how the scale moves from --cfg_scale at the first grid point to 1 at the last")
    p.add_argument("--cfg_rescale", type=float, default=0.0, metavar="PHI",
                   help="guidance rescale: blend PHI in [0, 1] of the guided output's std towards the prompt row's (0: off)")
    p.add_argument("--cfg_norm_limit", type=float, default=None, metavar="R",
                   help="cap the guided output's L2 norm per sample at R times the prompt row's (default: no limit)")
    p.add_argument("--apg_eta", type=float, default=None, metavar="ETA",
                   help="adaptive projected guidance (APG): the part of the guidance update parallel to the prompt row's output is scaled by "
                        "ETA (0 drops it, 1 keeps it; any --apg_* option switches APG on)")
    p.add_argument("--apg_momentum", type=float, default=None, metavar="BETA",
                   help="... the update carries BETA times the previous guided stage's update, |BETA| < 1 (the paper uses negative values)")
    p.add_argument("--apg_norm_threshold", type=float, default=None, metavar="R",
                   help="... and its L2 norm per sample is clipped to R (default: no clip)")
    p.add_argument("--cfg_zero_star", action="store_true",
                   help="CFG-Zero*: rescale the negative row's output by <prompt row, negative row> / |negative row|^2 before guidance")
    p.add_argument("--cfg_zero_init", type=int, default=0, metavar="K",
                   help="... and take zero velocity on the first K steps, which then evaluate nothing (needs --cfg_zero_star)")
    p.add_argument("--cfg_reuse", type=int, default=0, metavar="K",
                   help="take the guidance difference (prompt row - negative row) on every K-th guided stage and reuse it on the stages in "
                        "between, which then evaluate the prompt row alone (0: off)")
    p.add_argument("--cfg_reuse_per_step", action="store_true",
                   help="... instead on the first guided stage of every step (midpoint, rk4), reused on the step's other stages")
    p.add_argument("--slg_layers", type=int, nargs="+", default=None, metavar="L",
                   help="skip-layer guidance: the blocks a third evaluation of the prompt row leaves out (default: off)")
    p.add_argument("--slg_scale", type=float, default=0.0, metavar="S",
                   help="... whose prediction the guided output is pushed away from: + S * (prompt row - skip row) (0: off)")
    p.add_argument("--slg_interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="... on the stages with LO <= t < HI only (t = 0 noise, 1 data; default: all stages)")
    p.add_argument("--pag_layers", type=int, nargs="+", default=None, metavar="L",
                   help="perturbed-attention guidance: the blocks a third evaluation of the prompt row runs with the identity as their "
                        "self-attention map (default: off; --slg_layers beside it: blocks the same evaluation leaves out)")
    p.add_argument("--pag_scale", type=float, default=0.0, metavar="S",
                   help="... whose prediction the guided output is pushed away from: + S * (prompt row - perturbed row) (0: off)")
    p.add_argument("--pag_interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="... on the stages with LO <= t < HI only (t = 0 noise, 1 data; default: all stages)")
    p.add_argument("--seg_layers", type=int, nargs="+", default=None, metavar="L",
                   help="smoothed-energy guidance: the blocks a third evaluation of the prompt row runs on Gaussian-blurred queries "
                        "(default: off; --slg_layers beside it: blocks the same evaluation leaves out)")
    p.add_argument("--seg_scale", type=float, default=0.0, metavar="S",
                   help="... whose prediction the guided output is pushed away from: + S * (prompt row - blurred row) (0: off)")
    p.add_argument("--seg_sigma", type=float, default=None, metavar="SIGMA",
                   help="... the width of the blur over the token grid, in tokens (> 0; inf: every query becomes the mean query)")
    p.add_argument("--seg_interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="... on the stages with LO <= t < HI only (t = 0 noise, 1 data; default: all stages)")
    p.add_argument("--teacache", type=float, default=None, metavar="THR",
                   help="step caching (the TeaCache rule): leave the block stack out of an evaluation while the accumulated relative change of its "
                        "first-block input stays below THR, and add the residual the stack produced the last time it ran (default: off)")
    p.add_argument("--teacache_coefficients", type=float, nargs=5, default=None, metavar=("C4", "C3", "C2", "C1", "C0"),
                   help="... the polynomial the relative change goes through before it is accumulated, highest power first (default: identity)")
    p.add_argument("--tile", type=int, nargs=2, default=None, metavar=("H", "W"),
                   help="tiled (MultiDiffusion) sampling: --resolution names the canvas, the model runs on overlapping windows of H x W pixels "
                        "whose predictions are averaged where they overlap (one engine call per image)")
    p.add_argument("--tile_stride", type=int, nargs=2, default=None, metavar=("SH", "SW"), help="window stride in pixels (default: half the tile)")
    p.add_argument("--tile_weights", type=str, default="uniform", choices=["uniform", "cosine"],
                   help="weight of a window's pixels in the average: uniform, or a cosine bump that fades towards the window's border")
    p.add_argument("--compose_prompts", type=str, nargs="+", default=None, metavar="P",
                   help="composed guidance: every image is guided by these K <= 7 prompts at once, g = u + sum_k W_k (c_k - u), in place of the "
                        "caption file's line (which still names the output); the negative (empty) prompt is the base row u; one engine call "
                        "per image")
    p.add_argument("--compose_weights", type=float, nargs="+", default=None, metavar="W",
                   help="... the weight of each prompt, as many as prompts; a negative weight pushes away from its prompt")
    p.add_argument("--compose_interval", type=float, nargs=3, action="append", default=None, metavar=("K", "LO", "HI"),
                   help="... prompt K (counted from 1) weighs 0 at the stages whose time is not in [LO, HI) (may be given once per prompt)")
    p.add_argument("--num_sampling_steps", type=int, default=250)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--ckpt", type=str, required=True)
    p.add_argument("--precision", type=str, choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--ema", action="store_true", default=True)
    p.add_argument("--no-ema", dest="ema", action="store_false")
    p.add_argument("--image_save_path", type=str, default="samples")
    p.add_argument("--time_shifting_factor", type=float, default=1.0)
    p.add_argument("--caption_path", type=str, default="prompts.txt")
    p.add_argument("--resolution", type=str, default=[], nargs="+")
    p.add_argument("--proportional_attn", type=lambda v: str(v).lower() not in ("0", "false", "no"), default=True)
    p.add_argument("--scaling_method", type=str, default="Time-aware")
    p.add_argument("--scaling_watershed", type=float, default=0.3)
    p.add_argument("--debug", action="store_true", help="random-init weights (no checkpoint load), as in the reference")
    p.add_argument("--text_encoder", type=str, default="google/gemma-2b", help="local path of the text encoder (no network)")
    p.add_argument("--vae", type=str, default="", help="local path of the diffusers AutoencoderKL weights; empty: save latents")
    g = p.add_argument_group("Transport arguments")
    g.add_argument("--path-type", type=str, default="Linear", choices=["Linear", "GVP", "VP"])
    g.add_argument("--prediction", type=str, default="velocity", choices=["velocity", "score", "noise"])
    g.add_argument("--loss-weight", type=none_or_str, default=None, choices=[None, "velocity", "likelihood"])
    g.add_argument("--sample-eps", type=float)
    g.add_argument("--train-eps", type=float)
    g = p.add_argument_group("ODE arguments")
    g.add_argument("--sampling-method", "--solver", type=str, default="euler",
                   help="euler, midpoint, rk4, heun2, heun3, the adaptive dopri5 family, or a multistep method ab2 / ab3 / abm2 / abm3 (one model "
                        "evaluation per step)")
    g.add_argument("--atol", type=float, default=1e-6)
    g.add_argument("--rtol", type=float, default=1e-3)
    g.add_argument("--reverse", action="store_true")
    return p


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
