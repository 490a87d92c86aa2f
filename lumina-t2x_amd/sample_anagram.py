"""Multi-view (visual-anagram) illusions on the MI355X engine: Phase Init of the reference's ``visual_anagrams/generate.py`` (:341-418).

    prompt_j (style + description), negative prompt --[text encoder, hidden_states[-2]]--> rows j and V + j of cap_feats [2V, T, D]
    z ~ N(0, I) [1, 4, w/8, h/8] --[NextDiT.sample_views: ONE lt_sample_views call, every stage one forward_with_cfg of 2 V rows]--> latent
    latent / vae_scale --[VAE decoder]--> sample_<size>.png and sample_<size>.views.png (the image under every view)

Argument names follow the reference (``--prompts --views --view_args --style --num_inference_steps --time_shifting_factor --cfg_scale
--seed --resolution --name --save_dir --num_samples``).  The text encoder and the VAE stay third-party and are loaded from LOCAL paths, or
injected (``run(args, encode_fn=..., decode_fn=..., model=...)``) exactly as ``sample.py`` allows; without a VAE the latent is written as
``latent_<size>.pt`` and no image.  The latent is always written.

Not built, and refused by name: Phase Upscale of generate.py (:437-494, ``--upscale``) - it needs the tiled VAE and switches on
proportional attention / time-aware scaling, where the anagram fork of the model is a different function from every model the engine
implements; animation (animate.py); views that are not pixel permutations (``lumina_t2x_amd.views``).

    python -m lumina_t2x_amd.sample_anagram --name duck_rabbit --ckpt /ckpts/Lumina-Next-SFT --text_encoder /ckpts/gemma-2b \\
        --vae /ckpts/sdxl-vae --prompts "a duck" "a rabbit" --views identity rotate_cw --style "an oil painting of" \\
        --num_inference_steps 30 --time_shifting_factor 4 --resolution 1024:1024x1024
"""
from __future__ import annotations

import argparse
import json
import os
from typing import List

import torch

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


def run(args, *, encode_fn=None, cap_feat_dim=None, decode_fn=None, model=None, train_args=None) -> List[dict]:
    """``encode_fn`` / ``decode_fn`` / ``model`` / ``train_args`` (the namespace of ``model_args.pth``: ``model``, ``qk_norm``, ``image_size``,
    ``vae``) can be injected; otherwise they are built from the command-line paths."""
    torch.set_grad_enabled(False)
    if getattr(args, "upscale", False):
        raise NotImplementedError("Phase Upscale (generate.py:437-494, midpoint_solver_extra) is not built: it needs the tiled VAE and the anagram "
                                  "fork's proportional-attention / time-aware-scaling model, which the engine does not implement")
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
    p.add_argument("--upscale", action="store_true", help="Phase Upscale of the reference: refused (not built)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.view_args is not None:
        args.view_args = [None if a == "None" else a for a in args.view_args]
    run(args)


if __name__ == "__main__":
    main()
