"""Prompt-driven image editing driver on the MI355X engine: FlowEdit's inversion-free rule (Kulikov et al., 2024).  Not in the
reference; loaders, arguments and output layout are those of ``sample_img2img.py``.

    input image --[resize, [-1, 1], VAE encoder]--> x_src = latent * vae_scale
    grid = ODE(num_sampling_steps, "euler", time_shifting_factor, strength=...).t       (cut exactly as img2img cuts it; the edit starts there)
    z = x_src;  one noise draw per interval;  rows = [source caption, target caption, negative, negative]
    z = model.sample_flowedit(x_src, grid[: n - n_min + 1], noise, feats, mask, src_cfg, tgt_cfg)          ONE lt_sample_flowedit call
    --n_min K > 0: the last K intervals are ordinary guided sampling of the target prompt from
        transport.edit.edit_tail_start(z, x_src, one more draw, t)  through ODE.sample                      ONE lt_sample_ode call
    --[VAE decoder]--> png + data.json (scales, cut, seed)

``--caption_path`` lists the TARGET captions, one edit each; ``--source_caption`` describes the input image.  Averaging over several noise draws
per interval (``n_avg`` in the paper) is not served.  The text encoder and the VAE can be injected (tests; callers that already hold them).

    python -m lumina_t2x_amd.sample_edit --ckpt /ckpts/Lumina-Next-SFT --image in.png --source_caption "a cat on a sofa" \\
        --caption_path targets.txt --src_cfg 1.5 --tgt_cfg 5.5 --strength 0.7 --num_sampling_steps 30 --time_shifting_factor 4 \\
        --resolution 1024:1024x1024 --text_encoder /ckpts/gemma-2b --vae /ckpts/sdxl-vae
"""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import Callable, List, Optional

import torch

from . import models
from .sample import VAE_SCALE, load_checkpoint, load_train_args, make_text_encoder, parse_resolution, save_png
from .sample_img2img import load_image, make_vae
from .transport import edit as E
from .transport.mini import ODE


def edit_grids(num_steps: int, time_shifting_factor, strength: float, n_min: int):
    """(the cut grid, the edit's part of it, the tail's part or None): the last ``n_min`` intervals belong to the tail"""
    grid = ODE(num_steps, "euler", time_shifting_factor, strength=strength).t
    n = len(grid) - 1
    if n < 1:
        raise ValueError(f"strength {strength} with {num_steps} steps leaves no interval to integrate")
    if not 0 <= n_min < n:
        raise ValueError(f"--n_min {n_min} must lie in 0..{n - 1}: the cut grid has {n} intervals and the edit needs at least one")
    return grid, grid[: n - n_min + 1], (grid[n - n_min:] if n_min else None)


def run(args, *, encode_fn=None, cap_feat_dim=None, vae_encode_fn: Optional[Callable] = None, decode_fn=None, model=None,
        image: Optional[torch.Tensor] = None) -> List[dict]:
    torch.set_grad_enabled(False)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    # (without a ROCm device only an injected model that is not engine-backed runs: the host loop)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0"))) if torch.cuda.is_available() else torch.device("cpu")
    if device.type == "cuda":
        torch.cuda.set_device(device)
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[args.precision]
    grid, edit_grid, tail_grid = edit_grids(args.num_sampling_steps, args.time_shifting_factor, args.strength, args.n_min)
    train_args = load_train_args(args.ckpt)
    if encode_fn is None:
        encode_fn, cap_feat_dim = make_text_encoder(args.text_encoder, dtype, device)
    if model is None:
        model = models.__dict__[train_args.model](qk_norm=train_args.qk_norm, cap_feat_dim=cap_feat_dim)
        model.eval().to(device, dtype=dtype)
        if not args.debug:
            model.load_state_dict(load_checkpoint(args.ckpt, args.ema), strict=True)
    if vae_encode_fn is None or decode_fn is None:
        enc, dec = make_vae(args.vae, device)
        vae_encode_fn = vae_encode_fn or enc
        decode_fn = decode_fn or dec
    if vae_encode_fn is None:
        raise RuntimeError("editing needs a VAE ENCODER for the input image: pass --vae <local diffusers AutoencoderKL> (diffusers must be "
                           "installed) or inject vae_encode_fn")
    out_dir = args.image_save_path
    os.makedirs(os.path.join(out_dir, "images"), exist_ok=True)
    with open(args.caption_path, "r", encoding="utf-8") as f:
        captions = [ln.strip() for ln in f if ln.strip()]
    factor = VAE_SCALE.get(getattr(train_args, "vae", "sdxl"), 0.18215)
    n_edit = len(edit_grid) - 1
    info: List[dict] = []
    jobs = [(res, i, c) for res in args.resolution for i, c in enumerate(captions)]
    for j, (res, idx, caption) in enumerate(jobs):
        if j % world != rank:
            continue
        cat, w, h = parse_resolution(res)
        if int(args.seed) != 0:
            torch.random.manual_seed(int(args.seed))
        img = image if image is not None else load_image(args.image, w, h, device)
        x_src = vae_encode_fn(img[None] if img.dim() == 3 else img).mul(factor).to(dtype)
        if tuple(x_src.shape) != (1, 4, h // 8, w // 8):
            raise ValueError(f"VAE latent {tuple(x_src.shape)} does not match the requested resolution {w}x{h} (expected [1, 4, {h // 8}, {w // 8}])")
        noise = torch.randn([n_edit, 1, 4, h // 8, w // 8], device=device).to(dtype)
        feats, mask = encode_fn([args.source_caption, caption, args.negative_caption, args.negative_caption])
        mask = mask.to(feats.device)
        kw = dict(proportional_attn=bool(args.proportional_attn), base_seqlen=(train_args.image_size // 16) ** 2 if args.proportional_attn else None)
        if cat > 1024 and args.scaling_method == "Time-aware":
            kw.update(scale_factor=math.sqrt(w * h / train_args.image_size ** 2), scale_watershed=args.scaling_watershed)
        else:
            kw.update(scale_factor=1.0, scale_watershed=1.0)
        latent = E.edit(model, x_src, edit_grid, noise, (feats, mask), args.src_cfg, args.tgt_cfg, **(kw if hasattr(model, "sample_flowedit") else {}))
        if tail_grid is not None:  # ordinary guided sampling of the target prompt over the last n_min intervals
            start = E.edit_tail_start(latent, x_src, torch.randn([1, 4, h // 8, w // 8], device=device).to(dtype), float(tail_grid[0]))
            tail = ODE(args.num_sampling_steps, "euler", args.time_shifting_factor)
            tail.t = tail_grid
            rows = [1, 3]  # the target caption and its negative
            latent = tail.sample(start.repeat(2, 1, 1, 1), model.forward_with_cfg, cap_feats=feats[rows].contiguous(),
                                 cap_mask=mask[rows].contiguous(), cfg_scale=args.tgt_cfg, **kw)[-1][:1]
        stem = os.path.join(out_dir, "images", f"edit_{args.num_sampling_steps}_{idx}_{res.split(':')[-1]}")
        if decode_fn is not None:
            save_png(decode_fn(latent / factor)[0], stem + ".png")
            url = stem + ".png"
        else:
            torch.save(latent.cpu(), stem + ".pt")
            url = stem + ".pt"
        info.append({"caption": caption, "source_caption": args.source_caption, "negative_caption": args.negative_caption, "image_url": url,
                     "resolution": f"res: {res.split(':')[-1]}\ntime_shift: {args.time_shifting_factor}", "solver": "flowedit-euler",
                     "num_sampling_steps": args.num_sampling_steps, "src_cfg": args.src_cfg, "tgt_cfg": args.tgt_cfg, "strength": args.strength,
                     "t_start": float(grid[0]), "intervals": len(grid) - 1, "n_min": args.n_min, "seed": int(args.seed)})
    with open(os.path.join(out_dir, f"data.rank{rank}.json" if world > 1 else "data.json"), "w") as f:
        json.dump(info, f)
    return info


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--image", type=str, required=True)
    p.add_argument("--source_caption", type=str, required=True, help="what the input image shows")
    p.add_argument("--caption_path", type=str, default="prompts.txt", help="the target captions, one edit per line")
    p.add_argument("--negative_caption", type=str, default="", help="the negative prompt of both branches")
    p.add_argument("--src_cfg", type=float, default=1.5, help="guidance scale of the source branch")
    p.add_argument("--tgt_cfg", type=float, default=5.5, help="guidance scale of the target branch (and of the --n_min tail)")
    p.add_argument("--strength", type=float, default=0.7, help="cuts the time grid as img2img does: the edit starts at t[int(n (1 - strength))]")
    p.add_argument("--n_min", type=int, default=0, help="the last K intervals are ordinary guided sampling of the target prompt")
    p.add_argument("--num_sampling_steps", type=int, default=30)
    p.add_argument("--time_shifting_factor", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--ckpt", type=str, required=True)
    p.add_argument("--precision", type=str, choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--ema", action="store_true", default=True)
    p.add_argument("--no-ema", dest="ema", action="store_false")
    p.add_argument("--image_save_path", type=str, default="samples")
    p.add_argument("--resolution", type=str, default=[], nargs="+")
    p.add_argument("--proportional_attn", type=lambda v: str(v).lower() not in ("0", "false", "no"), default=True)
    p.add_argument("--scaling_method", type=str, default="Time-aware")
    p.add_argument("--scaling_watershed", type=float, default=0.3)
    p.add_argument("--debug", action="store_true", help="random-init weights (no checkpoint load)")
    p.add_argument("--text_encoder", type=str, default="google/gemma-2b", help="local path of the text encoder (no network)")
    p.add_argument("--vae", type=str, default="", help="local path of the diffusers AutoencoderKL weights (encoder AND decoder)")
    return p


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
