"""View synthesis on the device: a view pushed forward through its disparity map to another
point on the baseline, and the disparity-scale augmentation built on it.

The reference augments its aerial data offline (``dataloaders/augmentations/new_tagil_aug.py``:
warp_aug -> warp_right_from_right): with probability ``warp_prob`` it re-synthesises the right view
at a random baseline fraction ``scale`` in 1 +- ``max_scale_diff`` from the right image and the
right disparity, scales the left target by ``scale``, and writes the dataset back to disk once
per variant.  Here the host only draws the random numbers, in the reference's order;
``kernels.forward_warp`` renders the whole batch in one launch, so every step sees a fresh scale.

  * ``view_from_left`` / ``view_from_right``  the scene from baseline fraction ``s`` (0 = the left
    camera, 1 = the right one; beyond either is legal)
  * ``sample_warp_scale``                     warp_aug's draws -> (chosen, scale)
  * ``DisparityScaleAugment``                 a standardised batch -> ``ScaledPair``

The warp is the 1-D mesh render of ``lea_forward_warp_f32`` (include/leastereo_hip.h), not the
reference's rounded point splat with a median over its cracks: sub-pixel exact, crack-free on
slanted surfaces, the same bits call after call.
"""
from __future__ import annotations

import collections
import random

import torch

from . import kernels

ScaledPair = collections.namedtuple("ScaledPair", "left right disp_left state scales chosen")
ScaledPair.__doc__ = """What ``DisparityScaleAugment`` returns, on the device: ``left`` (the input), ``right``
(re-synthesised where chosen, the input bit for bit elsewhere), ``disp_left`` (times the scale where chosen),
``state`` uint8 [B, H, W] (1 where the new right view is synthetic fill, 0 elsewhere and in samples not
chosen), ``scales`` float32 [B] (1 where not chosen) and ``chosen`` bool [B]."""


def view_from_left(left: torch.Tensor, disp_left: torch.Tensor, s=1.0, **kw) -> kernels.WarpedView:
    """The scene of ``left`` [B, C, H, W] seen from baseline fraction ``s`` (a float or a [B]
    float32 device tensor): left pixel x with disparity d lands on x - s d.  ``s = 1`` is the
    right camera, ``s = 0`` the identity.  ``kw`` goes to ``kernels.forward_warp``."""
    return kernels.forward_warp(left, disp_left, scale=s, **kw)


def view_from_right(right: torch.Tensor, disp_right: torch.Tensor, s=0.0, **kw) -> kernels.WarpedView:
    """The same from the right view and its own disparity: right pixel u with disparity d_r is
    seen from baseline fraction ``s`` at u - (s - 1) d_r, so ``s = 1`` is the identity and
    ``s = 0`` lands in the left view."""
    return kernels.forward_warp(right, disp_right, scale=s - 1.0, **kw)  # a tensor: one float32 subtraction each


def sample_warp_scale(prob, max_scale_diff, rng=random):
    """warp_aug's draws, in its order and count: one ``rng.random()`` for the choice, as
    ``choose([1 - prob, prob])`` makes it (chosen unless the draw is below 1 - prob), and only if
    chosen a second one for ``1 + (2 r - 1) max_scale_diff``.  Returns ``(chosen, scale)``, the
    scale 1.0 when not chosen."""
    if not rng.random() < 1 - prob:
        return True, 1 + (2 * rng.random() - 1) * max_scale_diff
    return False, 1.0


class DisparityScaleAugment:
    """The reference's disparity-scale augmentation for a whole batch, online and on the device.

    Call it on standardised float batches (``TrainBatch.left`` / ``right`` / ``target`` are that):
    ``left``, ``right`` float32 [B, C, H, W], ``disp_left`` float32 [B, H, W].

      * with ``disp_right`` [B, H, W]: the new right view is ``view_from_right(right, disp_right,
        scales)``, the reference's path; it keeps the real right image and its holes are only
        |scale - 1| disparities wide
      * without: ``view_from_left(left, disp_left, scales)``, stereo from a single image.  Such a
        ``disp_left`` must be dense; a sparse target is densified on the device by
        ``kernels.fgs_refine`` first, and what stays unknown goes in as ``exclude``

    One launch for the batch.  A scale is drawn per sample in batch order (``rng``: anything with
    ``random()``; None is the ``random`` module, as in the reference) and uploaded without
    blocking.  Samples not chosen keep their right image and target bit for bit (a select on the
    device, no synchronisation); chosen ones get ``disp_left * scale``, one float32 multiply,
    where the target is valid (> 0.001 and, with ``maxdisp``, below it) -- an invalid target
    keeps its bits and stays invalid.  ``warp_kw`` goes to ``kernels.forward_warp``."""

    def __init__(self, prob=0.5, max_scale_diff=0.3, rng=None, device="cuda", maxdisp=None, **warp_kw):
        if not 0 <= prob <= 1 or not 0 <= max_scale_diff:
            raise ValueError(f"DisparityScaleAugment: bad prob {prob} or max_scale_diff {max_scale_diff}")
        self.prob, self.max_scale_diff = float(prob), float(max_scale_diff)
        self.rng = random if rng is None else rng
        self.device = torch.device(device)
        self.maxdisp = None if maxdisp is None else float(maxdisp)
        self.warp_kw = dict(warp_kw)
        self.warp_kw.setdefault("want_zview", False)

    def sample(self, b):
        """The [2, B] float32 host tensor of one batch's draws: row 0 the scales, row 1 chosen
        as 1 / 0 (pinned when a ROCm device is there)."""
        draws = [sample_warp_scale(self.prob, self.max_scale_diff, self.rng) for _ in range(b)]
        p = torch.tensor([[s for _, s in draws], [1.0 if c else 0.0 for c, _ in draws]], dtype=torch.float32)
        return p.pin_memory() if torch.cuda.is_available() else p

    def __call__(self, left, right, disp_left, disp_right=None, exclude=None) -> ScaledPair:
        if left.dim() != 4 or left.shape != right.shape or disp_left.shape != left.shape[:1] + left.shape[2:]:
            raise ValueError(f"DisparityScaleAugment: left / right must be [B, C, H, W] and disp_left [B, H, W], got "
                             f"{tuple(left.shape)}, {tuple(right.shape)} and {tuple(disp_left.shape)}")
        b = left.shape[0]
        p = self.sample(b).to(left.device, non_blocking=True)
        scales, chosen = p[0].contiguous(), p[1] != 0
        if disp_right is not None:
            view = view_from_right(right, disp_right, scales, exclude=exclude, want_state=True, **self.warp_kw)
        else:
            view = view_from_left(left, disp_left, scales, exclude=exclude, want_state=True, **self.warp_kw)
        new_right = torch.where(chosen[:, None, None, None], view.image, right)
        state = torch.where(chosen[:, None, None], view.state, torch.zeros_like(view.state))
        valid = disp_left > 0.001
        if self.maxdisp is not None:
            valid &= disp_left < self.maxdisp
        target = torch.where(valid & chosen[:, None, None], disp_left * scales[:, None, None], disp_left)
        return ScaledPair(left, new_right, target, state, scales, chosen)
