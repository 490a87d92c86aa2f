"""Multi-view (visual-anagram) illusions on the MI355X engine: Phase Init of the reference's ``visual_anagrams/generate.py`` (:341-418) and,
with ``--upscale``, its Phase Upscale (:416-498).

    prompt_j (style + description), negative prompt --[text encoder, hidden_states[-2]]--> rows j and V + j of cap_feats [2V, T, D]
    z ~ N(0, I) [1, 4, w/8, h/8] --[NextDiT.sample_views: ONE lt_sample_views call, every stage one forward_with_cfg of 2 V rows]--> latent
    latent / vae_scale --[VAE decoder]--> sample_<size>.png and sample_<size>.views.png (the image under every view)

Argument names follow the reference (``--prompts --views --view_args --style --num_inference_steps --time_shifting_factor --cfg_scale
--seed --resolution --name --save_dir --num_samples``).  The text encoder and the VAE stay third-party and are loaded from LOCAL paths, or
injected (``run(args, encode_fn=..., decode_fn=..., model=...)``) exactly as ``sample.py`` allows; without a VAE the latent is written as
``latent_<size>.pt`` and no image.  The latent is always written.

``--upscale`` continues as generate.py:416-498 does:
    latent --[VAE decoder]--> image --[bicubic F.interpolate to (h, w), fp32]--> --[VAE encoder]--> guidance latent [1, 4, h/8, w/8]
    z' ~ N(0, I) like it --[NextDiT.sample_views_guided: ONE lt_sample_views_guided call, the anagram fork's attention rule]--> latent
    --[VAE decoder]--> upscaled_<size>.png, upscaled_<size>.views.png, upscaled_latent_<size>.pt
with ``--proportional_attn``, ``--scaling_method`` and ``--scaling_watershed`` read as generate.py:420-435 reads them (the fork's model ignores
the watershed).  The VAE stays third-party here as everywhere in this project: the codec encodes and decodes the WHOLE image - the reference's
tiled passes (``tiled_encode`` / ``tiled_decode``, generate.py:60-173) are not rebuilt.  Phase Upscale needs a VAE encoder (``--vae`` with
diffusers, or ``vae_encode_fn``); without one ``--upscale`` is refused by name.

Not built, and refused by name: animation (animate.py); views that are not pixel permutations (``lumina_t2x_amd.views``).

    python -m lumina_t2x_amd.sample_anagram --name duck_rabbit --ckpt /ckpts/Lumina-Next-SFT --text_encoder /ckpts/gemma-2b \\
        --vae /ckpts/sdxl-vae --prompts "a duck" "a rabbit" --views identity rotate_cw --style "an oil painting of" \\
        --num_inference_steps 30 --time_shifting_factor 4 --resolution 1024:1024x1024
"""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import List

import torch
import torch.nn.functional as F

from . import models
from .sample import VAE_SCALE, load_checkpoint, load_train_args, make_text_encoder, make_vae_decoder, parse_resolution, save_png
from .views import get_anagrams_views

DEFAULT_NEGATIVE = "blurry, low quality, distorted, watermark"


def time_grid(num_inference_steps: int, time_shifting_factor: float) -> List[float]:
    """generate.py:378-385: linspace(0, 1, n) in fp32, shifted t / (t + s - s t), as Python floats"""
    t = torch.linspace(0.0, 1.0, num_inference_steps)
    if time_shifting_factor:
        t = t / (t + time_shifting_factor - time_shifting_factor * t)
    return t.tolist()


def encode_views(encode_fn, prompts: List[str], style: str, negative: str):
    """the V (style + prompt) captions and the negative caption in ONE padded batch, laid out as forward_with_cfg wants 2 V rows:
    rows 0..V-1 the view prompts, rows V..2V-1 the negative prompt (the reference encodes V pairs [prompt_j, negative], generate.py:344-351;
    padding is masked, so the common length changes nothing)"""
    caps = [f"{style} {p}".strip() for p in prompts]
    feats, mask = encode_fn(caps + [negative])
    V = len(caps)
    rows = list(range(V)) + [V] * V
    return feats[rows].contiguous(), mask[rows].contiguous()


def make_vae_encoder(path, device):
    """image in [-1, 1] -> a sample of the latent distribution (NOT yet multiplied by the scale factor), as generate.py:91 draws it; None when
    diffusers / the weights are unavailable.  The whole image in one pass (no tiling)."""
    if not path:
        return None
    try:
        from diffusers.models import AutoencoderKL
    except ImportError:
        return None
    vae = AutoencoderKL.from_pretrained(path, torch_dtype=torch.float32).to(device).eval()

    @torch.no_grad()
    def encode(image):
        return vae.encode(image.float()).latent_dist.sample()

    return encode


def upscale_model_kwargs(args, cat: int, w: int, h: int, image_size: int) -> dict:
    """generate.py:420-435 (and :369: do_extrapolation); the fork's model ignores scale_watershed, so it is not handed on"""
    kw = dict(proportional_attn=bool(args.proportional_attn), base_seqlen=(image_size // 16) ** 2 if args.proportional_attn else None, scale_factor=1.0)
    if cat > image_size and args.scaling_method == "Time-aware":
        kw["scale_factor"] = math.sqrt(w * h / image_size ** 2)
    return kw


def run(args, *, encode_fn=None, cap_feat_dim=None, decode_fn=None, model=None, train_args=None, vae_encode_fn=None) -> List[dict]:
    """``encode_fn`` / ``decode_fn`` / ``vae_encode_fn`` / ``model`` / ``train_args`` (the namespace of ``model_args.pth``: ``model``, ``qk_norm``,
    ``image_size``, ``vae``) can be injected; otherwise they are built from the command-line paths.  ``vae_encode_fn``: image ``[1, 3, h, w]`` in
    [-1, 1] -> latent ``[1, 4, h / 8, w / 8]`` before the scale factor (``--upscale`` only; the whole image, no tiling)."""
    torch.set_grad_enabled(False)
    upscale = bool(getattr(args, "upscale", False))
    if upscale and vae_encode_fn is None and not args.vae:
        raise NotImplementedError("Phase Upscale (generate.py:437-494) needs a VAE encoder for the guidance latent and none is available: pass --vae "
                                  "(a local diffusers AutoencoderKL) or inject vae_encode_fn")
    if len(args.prompts) != len(args.views):
        raise ValueError("Number of prompts must match number of views")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[args.precision]
    if train_args is None:
        train_args = load_train_args(args.ckpt)
    image_size = getattr(train_args, "image_size", 1024)
    if encode_fn is None:
        encode_fn, cap_feat_dim = make_text_encoder(args.text_encoder, dtype, device)
    if model is None:
        model = models.__dict__[train_args.model](qk_norm=train_args.qk_norm, cap_feat_dim=cap_feat_dim)
        model.eval().to(device, dtype=dtype)
        if not args.debug:
            model.load_state_dict(load_checkpoint(args.ckpt, args.ema), strict=True)
    if decode_fn is None:
        decode_fn = make_vae_decoder(args.vae, device)
        if decode_fn is None:
            print("[sample_anagram] no VAE decoder (diffusers or --vae missing): writing latents only", flush=True)
    if upscale:
        if vae_encode_fn is None:
            vae_encode_fn = make_vae_encoder(args.vae, device)
        if vae_encode_fn is None or decode_fn is None:
            raise NotImplementedError("Phase Upscale (generate.py:437-494) needs a VAE encoder and decoder for the guidance latent and diffusers or the "
                                      "--vae weights are missing")
    factor = VAE_SCALE.get(getattr(train_args, "vae", "sdxl"), 0.18215)
    views = get_anagrams_views(args.views, view_args=args.view_args)
    cap_feats, cap_mask = encode_views(encode_fn, list(args.prompts), args.style, args.negative_prompt)
    cap_feats, cap_mask = cap_feats.to(device), cap_mask.to(device)
    save_dir = os.path.join(args.save_dir, args.name)
    os.makedirs(save_dir, exist_ok=True)
    grid = time_grid(args.num_inference_steps, args.time_shifting_factor)
    info: List[dict] = []
    for i in range(args.num_samples):
        torch.manual_seed(args.seed + i)  # generate.py:361
        sample_dir = os.path.join(save_dir, f"{args.seed + i:04}")
        os.makedirs(sample_dir, exist_ok=True)
        for res in args.resolution:
            cat, w, h = parse_resolution(res)
            scale = cat / image_size
            # generate.py:371-375 (width first, as the reference draws it)
            latent_w, latent_h = int(w / scale) // 8, int(h / scale) // 8
            z = torch.randn([1, 4, latent_w, latent_h], device=device).to(dtype)
            latent = model.sample_views(z, grid, views, cap_feats, cap_mask, "midpoint", cfg_scale=args.cfg_scale, return_trajectory=False)
            size = latent.shape[-1] * 8
            entry = {"prompts": list(args.prompts), "views": list(args.views), "view_args": args.view_args, "style": args.style,
                     "seed": args.seed + i, "resolution": res, "num_inference_steps": args.num_inference_steps,
                     "latent": os.path.join(sample_dir, f"latent_{size}.pt")}
            torch.save(latent.cpu(), entry["latent"])
            if decode_fn is not None:
                image = decode_fn(latent / factor)  # [1, 3, H, W] in [0, 1]
                entry["image"] = os.path.join(sample_dir, f"sample_{size}.png")
                save_png(image[0], entry["image"])
                # the image under every view, side by side (utils.save_illusion)
                entry["views_image"] = os.path.join(sample_dir, f"sample_{size}.views.png")
                save_png(torch.cat([v.view(image[0].float() * 2 - 1) / 2 + 0.5 for v in views], dim=2), entry["views_image"])
            if upscale:
                # generate.py:442-463: the decoded illusion, bicubic to (h, w) in fp32, rounded to bf16, encoded: the guidance latent; a fresh z
                guidance = F.interpolate(image.float() * 2 - 1, size=(h, w), mode="bicubic").to(torch.bfloat16)
                guidance = (vae_encode_fn(guidance) * factor).to(dtype)
                z = torch.randn_like(guidance[:1]).to(dtype)
                kw = upscale_model_kwargs(args, cat, w, h, image_size)
                up = model.sample_views_guided(z, guidance, grid, views, cap_feats, cap_mask, cfg_scale=args.cfg_scale,
                                               coef_rounding=args.coef_rounding, return_trajectory=False, **kw)
                usize = up.shape[-1] * 8
                entry.update(upscale=kw, upscaled_latent=os.path.join(sample_dir, f"upscaled_latent_{usize}.pt"),
                             upscaled_image=os.path.join(sample_dir, f"upscaled_{usize}.png"),
                             upscaled_views_image=os.path.join(sample_dir, f"upscaled_{usize}.views.png"))
                torch.save(up.cpu(), entry["upscaled_latent"])
                image = decode_fn(up / factor)
                save_png(image[0], entry["upscaled_image"])
                save_png(torch.cat([v.view(image[0].float() * 2 - 1) / 2 + 0.5 for v in views], dim=2), entry["upscaled_views_image"])
            info.append(entry)
    with open(os.path.join(save_dir, "metadata.json"), "w") as f:
        json.dump(info, f, indent=1)
    return info


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--name", required=True, type=str)
    p.add_argument("--save_dir", type=str, default="results")
    p.add_argument("--prompts", required=True, type=str, nargs="+", help="one prompt per view")
    p.add_argument("--views", required=True, type=str, nargs="+", help="view names (lumina_t2x_amd.views.VIEW_MAP)")
    p.add_argument("--view_args", default=None, type=str, nargs="+", help="one argument per view ('None' for none)")
    p.add_argument("--style", default="", type=str, help="optional string to prepend every prompt with")
    p.add_argument("--negative_prompt", default=DEFAULT_NEGATIVE, type=str)
    p.add_argument("--num_inference_steps", type=int, default=100)
    p.add_argument("--num_samples", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--cfg_scale", type=float, default=4.0)
    p.add_argument("--time_shifting_factor", type=float, default=1.0)
    p.add_argument("--resolution", type=str, default=["1024:1024x1024"], nargs="+")
    p.add_argument("--ckpt", type=str, default="")
    p.add_argument("--precision", type=str, choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--ema", action="store_true", default=True)
    p.add_argument("--no-ema", dest="ema", action="store_false")
    p.add_argument("--debug", action="store_true", help="random-init weights (no checkpoint load), as in the reference")
    p.add_argument("--text_encoder", type=str, default="google/gemma-2b", help="local path of the text encoder (no network)")
    p.add_argument("--vae", type=str, default="", help="local path of the diffusers AutoencoderKL weights; empty: latents only")
    p.add_argument("--upscale", action="store_true", help="continue with Phase Upscale of the reference (needs --vae: encoder and decoder)")
    p.add_argument("--proportional_attn", type=lambda v: str(v).lower() not in ("0", "false", "no", ""), default=True,
                   help="Phase Upscale: proportional attention with base_seqlen (image_size / 16)^2")
    p.add_argument("--scaling_method", type=str, default="Time-aware", help="Phase Upscale: 'Time-aware' scales the RoPE above the training size")
    p.add_argument("--scaling_watershed", type=float, default=0.3, help="accepted for the reference's command lines; its model ignores it")
    p.add_argument("--coef_rounding", type=str, choices=["fp32", "state"], default="fp32",
                   help="Phase Upscale: the decay factor multiplies the state in fp32 (expected of the reference's GPU run) or rounded to the state dtype")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.view_args is not None:
        args.view_args = [None if a == "None" else a for a in args.view_args]
    run(args)


if __name__ == "__main__":
    main()
