"""Views of a multi-view (visual-anagram) illusion: what ``visual_anagrams/visual_anagrams/views`` is to the reference's
``generate.py``, restricted to the views that are PIXEL PERMUTATIONS of the latent with a sign per channel.

Every class keeps the reference's interface on torch tensors - ``view(im)`` on a ``[C, H, W]`` latent, ``inverse_view(noise)`` on a noise
estimate - and adds ``table(h, w, channels=4) -> (perm, vsign, isign)``, the same view as data for the engine
(``DiTEngine.set_views`` -> ``lt_set_views``)::

    view(x)[c, i]          = vsign[c] * x[c].flatten()[perm[i]]
    inverse_view(n)[c, i]  = isign[c] * n[c].flatten()[iperm[i]],   iperm = inverse of perm (built on the device)

``perm`` is int32 ``[h * w]``, ``vsign`` / ``isign`` float32 ``[channels]`` of +-1.  The two signs are separate because the reference's
``NegateView`` negates every channel going in but only channels 0..2 coming back (views/view_negate.py:12-22); that quirk is kept.

``get_anagrams_views(view_names, view_args=None)`` has the reference's signature and names (views/__init__.py:23-77).  Views that are not
built are refused by name with the reason.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

__all__ = ["BaseView", "IdentityView", "FlipView", "Rotate90CWView", "Rotate90CCWView", "Rotate180View", "NegateView", "PatchPermuteView",
           "PermuteView", "VIEW_MAP", "UnsupportedViewError", "get_anagrams_views", "stack_tables"]


class UnsupportedViewError(ValueError):
    pass


class BaseView:
    """a pixel permutation with a sign per channel; subclasses give ``_index(h, w)`` (the source pixel of every output pixel)"""

    def _index(self, h: int, w: int) -> torch.Tensor:
        raise NotImplementedError

    def _signs(self, channels: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return torch.ones(channels), torch.ones(channels)

    def table(self, h: int, w: int, channels: int = 4) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        perm = self._index(int(h), int(w)).reshape(-1).to(torch.int32)
        if perm.numel() != h * w:
            raise ValueError(f"{type(self).__name__}: table of {perm.numel()} entries for a {h}x{w} latent")
        vs, isg = self._signs(channels)
        return perm, vs.to(torch.float32), isg.to(torch.float32)

    def _apply(self, x: torch.Tensor, inverse: bool) -> torch.Tensor:
        c, h, w = x.shape
        perm, vs, isg = self.table(h, w, c)
        idx = perm.to(device=x.device, dtype=torch.long)
        if inverse:
            inv = torch.empty_like(idx)
            inv[idx] = torch.arange(idx.numel(), device=idx.device)
            idx, sg = inv, isg
        else:
            sg = vs
        out = x.reshape(c, h * w)[:, idx].reshape(c, h, w)
        return out * sg.to(device=x.device, dtype=x.dtype).view(c, 1, 1)

    def view(self, im: torch.Tensor) -> torch.Tensor:
        return self._apply(im, False)

    def inverse_view(self, noise: torch.Tensor) -> torch.Tensor:
        return self._apply(noise, True)

    def make_frame(self, im, t):
        raise UnsupportedViewError(f"{type(self).__name__}.make_frame: animation (animate.py) is out of scope of this package")


def _grid(h: int, w: int) -> torch.Tensor:
    return torch.arange(h * w).view(h, w)


class IdentityView(BaseView):
    def _index(self, h, w):
        return _grid(h, w)


class FlipView(BaseView):
    """top <-> bottom (views/view_flip.py: torch.flip over the row axis)"""

    def _index(self, h, w):
        return _grid(h, w).flip(0)


class _Rot90(BaseView):
    k = 0

    def _index(self, h, w):
        if self.k % 2 and h != w:
            raise UnsupportedViewError(f"{type(self).__name__}: a 90 degree rotation needs a square latent, got {h}x{w}")
        return torch.rot90(_grid(h, w), self.k, dims=[0, 1])


class Rotate90CWView(_Rot90):
    k = -1


class Rotate90CCWView(_Rot90):
    k = 1


class Rotate180View(_Rot90):
    k = 2


class NegateView(BaseView):
    def _index(self, h, w):
        return _grid(h, w)

    def _signs(self, channels):
        vs = -torch.ones(channels)
        isg = torch.ones(channels)
        isg[:3] = -1  # the reference leaves the channels behind the third alone on the way back
        return vs, isg


class PatchPermuteView(BaseView):
    """random permutation of ``num_patches`` x ``num_patches`` square patches, drawn once with ``torch.randperm`` at construction
    (views/view_patch_permute.py); ``pixel_permute`` is this class with 64 patches per side"""

    def __init__(self, num_patches: int = 8):
        if num_patches < 1 or 64 % num_patches or 256 % num_patches:
            raise UnsupportedViewError(f"patch_permute: num_patches {num_patches} must divide 64 and 256")
        self.num_patches = int(num_patches)
        self.perm = torch.randperm(self.num_patches ** 2)

    def _index(self, h, w):
        n = self.num_patches
        if h != w or w % n:
            raise UnsupportedViewError(f"patch_permute: {n} patches per side need a square latent whose side is a multiple of {n}, got {h}x{w}")
        p = w // n
        patches = _grid(h, w).view(n, p, n, p).permute(0, 2, 1, 3).reshape(n * n, p, p)[self.perm]
        return patches.view(n, n, p, p).permute(0, 2, 1, 3).reshape(h, w)


class PermuteView(BaseView):
    """a caller-supplied pixel permutation: ``perm[i]`` = the source pixel of output pixel i (row-major over H x W).  This is how jigsaw,
    inner-circle or square-hinge tables made elsewhere are brought in."""

    def __init__(self, perm):
        perm = torch.as_tensor(perm).reshape(-1).to(torch.long)
        n = perm.numel()
        if n == 0 or not torch.equal(torch.sort(perm).values, torch.arange(n)):
            raise ValueError(f"PermuteView: the table is not a permutation of 0..{n - 1}")
        self.perm = perm

    def _index(self, h, w):
        if h * w != self.perm.numel():
            raise ValueError(f"PermuteView: table of {self.perm.numel()} pixels used on a {h}x{w} latent")
        return self.perm


VIEW_MAP = {
    "identity": IdentityView,
    "flip": FlipView,
    "rotate_cw": Rotate90CWView,
    "rotate_ccw": Rotate90CCWView,
    "rotate_180": Rotate180View,
    "negate": NegateView,
    "patch_permute": PatchPermuteView,
    "pixel_permute": PatchPermuteView,
}

_NEEDS_ASSETS = "its tables come from the reference's PNG assets / generators; build the table there and pass it as PermuteView(perm)"
_NOT_A_PERMUTATION = "it is not a pixel permutation of the latent (it filters, recolours or resamples), which is all the engine's view kernels move"
REFUSED = {
    "jigsaw": _NEEDS_ASSETS, "inner_circle": _NEEDS_ASSETS, "square_hinge": _NEEDS_ASSETS, "inner_circle_failure": _NEEDS_ASSETS,
    "skew": _NOT_A_PERMUTATION, "blur_failure": _NOT_A_PERMUTATION, "white_balance_failure": _NOT_A_PERMUTATION,
    "low_pass": _NOT_A_PERMUTATION, "high_pass": _NOT_A_PERMUTATION, "triple_low_pass": _NOT_A_PERMUTATION,
    "triple_medium_pass": _NOT_A_PERMUTATION, "triple_high_pass": _NOT_A_PERMUTATION, "grayscale": _NOT_A_PERMUTATION,
    "color": _NOT_A_PERMUTATION, "motion": _NOT_A_PERMUTATION, "motion_res": _NOT_A_PERMUTATION, "scale": _NOT_A_PERMUTATION,
}


def get_anagrams_views(view_names: Sequence[str], view_args: Optional[Sequence] = None) -> List[BaseView]:
    if view_args is None:
        view_args = [None for _ in view_names]
    views = []
    for name, arg in zip(view_names, view_args):
        if name in REFUSED:
            raise UnsupportedViewError(f"view '{name}' is not supported: {REFUSED[name]}")
        if name not in VIEW_MAP:
            raise UnsupportedViewError(f"unknown view '{name}' (built: {sorted(VIEW_MAP)})")
        if name == "patch_permute":
            args = [8 if arg is None else int(arg)]
        elif name == "pixel_permute":
            args = [64 if arg is None else int(arg)]
        else:
            args = []
        views.append(VIEW_MAP[name](*args))
    return views


def stack_tables(views: Sequence[BaseView], h: int, w: int, channels: int = 4):
    """(perm int32 [V, h*w], vsign float32 [V, C], isign float32 [V, C]) of a list of views"""
    tabs = [v.table(h, w, channels) for v in views]
    return torch.stack([t[0] for t in tabs]), torch.stack([t[1] for t in tabs]), torch.stack([t[2] for t in tabs])
