"""The training loader's per-sample transform on the device.

The reference standardises every decoded image on the host in float64
(``dataloaders/datasets/common.py:119-131``, set_rgb_layers) and then pads, random-crops,
optionally shifts the left view against the right and cuts the disparity target
(``common.py:43-91``, train_transform).  Here the host only draws the random numbers, in the
reference's order, and turns them into five ints per sample; ``kernels.train_transform_u8``
does the rest on the decoded uint8 images in two launches.

  * ``sample_train_params``  the draws of train_transform -> one params row
  * ``center_params``        test_transform's geometry (``common.py:94-116``) -> one params row
  * ``DeviceTrainTransform`` a batch of decoded samples -> ``TrainBatch`` on the device

A params row is ``(src_y0, src_x0_left, src_x0_right, target_sub, flags)``: output pixel
(y, x) of the left input and of the target reads source pixel (y + src_y0, x + src_x0_left),
the right input (y + src_y0, x + src_x0_right); outside the image is pad (0 in the images,
1000 in the left disparity, 0 in the right); ``target - target_sub``; flags bit 0 swaps the
pair (include/leastereo_hip.h, lea_train_transform_u8).
"""
from __future__ import annotations

import collections
import random

import numpy as np
import torch

from . import kernels

FLAG_SWAP = 1

TrainBatch = collections.namedtuple("TrainBatch", "left right target n_valid params")


def sample_train_params(h, w, crop_h, crop_w, use_left=True, left_right=False, shift=0, rng=random):
    """One sample's params row, drawing from ``rng.randint`` exactly as train_transform draws
    from ``random.randint`` (same bounds, same order, same count), so ``rng=random`` under
    ``random.seed(s)`` sees the reference's crops."""
    h, w, ch, cw, shift = int(h), int(w), int(crop_h), int(crop_w), int(shift)
    if min(h, w, ch, cw) <= 0 or shift < 0:
        raise ValueError(f"train_transform: bad image {h}x{w}, crop {ch}x{cw} or shift {shift}")
    if h < ch and w > cw:
        # common.py:65/77: random.randint(0, h - crop_height) over an empty range
        raise ValueError(f"train_transform: a {h}x{w} image is lower than the {ch}x{cw} crop and wider "
                         "(the reference fails with 'empty range')")
    # the canvas the image is pasted into, bottom-right (common.py:46-58)
    if h > ch and w <= cw:
        hc, wc = h + shift, cw + shift
    elif h <= ch and w <= cw:
        hc, wc = ch + shift, cw + shift
    else:
        hc, wc = h, w
    py, px = hc - h, wc - w
    if shift > 0:
        start_x = rng.randint(0, wc - cw)
        shift_x = rng.randint(-shift, shift)
        if start_x + shift_x < 0 or start_x + shift_x + cw > wc:
            shift_x = 0
        start_y = rng.randint(0, hc - ch)
        return (start_y - py, start_x + shift_x - px, start_x - px, shift_x, 0)
    if h <= ch and w <= cw:
        start_x = start_y = 0
    else:
        start_x = rng.randint(0, wc - cw)
        start_y = rng.randint(0, hc - ch)
    flags = 0
    if not use_left:
        coin = rng.randint(0, 1)  # drawn whether or not left_right is set
        if not (coin == 0 and left_right):
            flags = FLAG_SWAP
    return (start_y - py, start_x - px, start_x - px, 0, flags)


def center_params(h, w, crop_h, crop_w):
    """test_transform's window: the image at the bottom-right of the crop when it fits, else the
    centre crop at ``start = (size - crop) // 2``.  Raises where ``kernels.standardize_crop_u8``
    raises: an image that neither fits the crop nor covers it."""
    h, w, ch, cw = int(h), int(w), int(crop_h), int(crop_w)
    if min(h, w, ch, cw) <= 0:
        raise ValueError(f"test_transform: bad image {h}x{w} or crop {ch}x{cw}")
    if h <= ch and w <= cw:
        return (h - ch, w - cw, w - cw, 0, 0)
    if h < ch or w < cw:
        raise ValueError(f"test_transform: a {h}x{w} image neither fits a {ch}x{cw} crop nor covers it "
                         "(the reference's copy into the crop fails)")
    return ((h - ch) // 2, (w - cw) // 2, (w - cw) // 2, 0, 0)


def _to_device(x, dtype, device):
    if x is None:
        return None
    if isinstance(x, (list, tuple)):
        x = np.stack([np.asarray(i.cpu() if isinstance(i, torch.Tensor) else i) for i in x])
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dtype != dtype:
        raise ValueError(f"expected {dtype}, got {x.dtype}")
    return x if x.is_cuda else x.to(device, non_blocking=True)


class DeviceTrainTransform:
    """``DatasetFromList.__getitem__``'s transform for a whole batch, on the device.

    Call it with equally sized decoded samples: ``left``/``right`` uint8 [B, H, W, 3|4],
    ``disp_left`` (and optionally ``disp_right``) float32 [B, H, W]; tensors on the host or
    the device, numpy arrays, or lists of per-sample arrays.  The params are drawn per sample
    in batch order (``rng``: anything with ``randint(a, b)``; None is the ``random`` module,
    as in the reference) and uploaded without blocking.  ``training=False`` is the validation
    side: ``center_params``, no draws, the left disparity with pad 1000."""

    def __init__(self, crop_height, crop_width, maxdisp, use_left=True, left_right=False, shift=0, rng=None,
                 device="cuda"):
        self.crop_height, self.crop_width, self.maxdisp = int(crop_height), int(crop_width), float(maxdisp)
        self.use_left, self.left_right, self.shift = bool(use_left), bool(left_right), int(shift)
        self.rng = random if rng is None else rng
        self.device = torch.device(device)

    def sample(self, b, h, w, training=True):
        """The [B, 5] int32 host tensor of one batch's params (pinned when a ROCm device is there)."""
        if training:
            rows = [sample_train_params(h, w, self.crop_height, self.crop_width, self.use_left, self.left_right,
                                        self.shift, self.rng) for _ in range(b)]
        else:
            rows = [center_params(h, w, self.crop_height, self.crop_width)] * b
        p = torch.tensor(rows, dtype=torch.int32)
        return p.pin_memory() if torch.cuda.is_available() else p

    def __call__(self, left, right, disp_left, disp_right=None, training=True) -> TrainBatch:
        left, right = (_to_device(t, torch.uint8, self.device) for t in (left, right))
        disp_left, disp_right = (_to_device(t, torch.float32, self.device) for t in (disp_left, disp_right))
        if left.dim() != 4:
            raise ValueError(f"left/right must be [B, H, W, 3|4] uint8, got {tuple(left.shape)}")
        b, h, w, _ = left.shape
        params = self.sample(b, h, w, training).to(left.device, non_blocking=True)
        out_l, out_r, target, n_valid = kernels.train_transform_u8(
            left, right, disp_left, disp_right, params, self.crop_height, self.crop_width, self.maxdisp)
        return TrainBatch(out_l, out_r, target, n_valid, params)
