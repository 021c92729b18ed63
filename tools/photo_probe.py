#!/usr/bin/env python3
"""The photometric loss at the training shape (4 x 3 x 288x576), in one process:

  * the two launches (lea_photometric_f32 with its one-workgroup reduction, and
    lea_photometric_grad_f32) through the C ABI on one stream, and the whole
    ``losses.photometric_loss(...).backward()`` that wraps them;
  * the same loss composed from torch ops (F.grid_sample, five F.avg_pool2d, the SSIM
    arithmetic, a min-pool for the window mask and two masked means; forward and backward).

Warmed up, then ``--rounds`` alternating windows of ``--iters`` calls each, HIP events;
medians of the windows with their range.  Writes the lines to ``--out`` as well.

  python tools/photo_probe.py [--iters 20] [--rounds 9] [--out profiles/photo_probe.txt]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leastereo_amd import _lib, kernels, losses  # noqa: E402

SHAPES = [(4, 3, 288, 576)]
ALPHA, C1, C2 = 0.85, kernels.PHOTO_C1, kernels.PHOTO_C2


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def torch_loss(left, right, disp):
    b, c, h, w = left.shape
    xs = torch.arange(w, device=left.device, dtype=torch.float32).view(1, 1, w) - disp
    in_view = (xs >= 0) & (xs <= w - 1)
    gy = torch.linspace(-1, 1, h, device=left.device).view(1, h, 1).expand(b, h, w)
    grid = torch.stack([2 * xs / (w - 1) - 1, gy], -1)
    wp = F.grid_sample(right, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * in_view.unsqueeze(1)
    l1 = (left - wp).abs().mean(1)
    mx, my = F.avg_pool2d(left, 3, 1), F.avg_pool2d(wp, 3, 1)
    sx = F.avg_pool2d(left * left, 3, 1) - mx * mx
    sy = F.avg_pool2d(wp * wp, 3, 1) - my * my
    sxy = F.avg_pool2d(left * wp, 3, 1) - mx * my
    ssim = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))
    dssim = torch.clamp((1 - ssim) / 2, 0, 1).mean(1)
    v = in_view.float()
    vs = -F.max_pool2d(-v.unsqueeze(1), 3, 1).squeeze(1)
    return ((1 - ALPHA) * (l1 * v).sum() / v.sum().clamp(min=1) +
            ALPHA * (dssim * vs).sum() / vs.sum().clamp(min=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "photo_probe.txt"))
    a = ap.parse_args()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; microseconds, median of {a.rounds} alternating windows of {a.iters} "
        f"calls [min, max]; alpha {ALPHA}")
    for b, c, h, w in SHAPES:
        # a smooth scene and its shifted view, a disparity that is nearly right
        base = 3 * F.avg_pool2d(torch.randn(b, c, h, w + 64, device="cuda", generator=g), 9, 1, 4)
        right = base[..., 64:].contiguous()
        true = [8 + 12 * i for i in range(b)]                   # left[x] = right[x - d], d per sample
        left = torch.stack([base[i, :, :, 64 - d: 64 - d + w] for i, d in enumerate(true)])
        left = left + 0.05 * torch.randn(left.shape, device="cuda", generator=g)
        disp = torch.tensor(true, device="cuda", dtype=torch.float32).view(b, 1, 1) + \
            0.5 * torch.randn(b, h, w, device="cuda", generator=g)
        sums = torch.empty(4, device="cuda", dtype=torch.float64)
        ws = torch.empty(lib.lea_photometric_workspace_bytes(b, h, w) // 8, device="cuda", dtype=torch.float64)
        ddisp = torch.empty(b, h, w, device="cuda")
        scales = torch.tensor([1 - ALPHA, ALPHA], device="cuda")
        chw, hw = c * h * w, h * w
        lp, rp, dp = left.data_ptr(), right.data_ptr(), disp.data_ptr()

        def fwd():
            _lib.check(lib.lea_photometric_f32(lp, chw, rp, chw, dp, hw, None, 0, b, c, h, w, ALPHA, C1, C2,
                                               sums.data_ptr(), ws.data_ptr(), None, None, stream), "sums")

        def bwd():
            _lib.check(lib.lea_photometric_grad_f32(lp, chw, rp, chw, dp, hw, None, 0, b, c, h, w, C1, C2,
                                                    sums.data_ptr(), scales.data_ptr(), ddisp.data_ptr(), hw, stream),
                       "grad")

        d_hip = disp.clone().requires_grad_()
        d_torch = disp.clone().requires_grad_()

        def wrapped():
            d_hip.grad = None
            losses.photometric_loss(left, right, d_hip).backward()

        def composed():
            d_torch.grad = None
            torch_loss(left, right, d_torch).backward()

        fns = (fwd, bwd, wrapped, composed)
        for fn in fns:
            fn()
            _timed(fn, a.iters)
        lh, lt = float(losses.photometric_loss(left, right, disp)), float(torch_loss(left, right, disp))
        # grid_sample rebuilds xs from a normalised coordinate: where that lands in the next
        # cell the slope is another one, so the largest difference is a whole gradient
        gerr = (d_hip.grad - d_torch.grad).abs().flatten()
        gdiff, gmax = float(gerr.max()), float(d_hip.grad.abs().max())
        g999 = float(gerr.kthvalue(int(0.999 * gerr.numel())).values)
        s = sums.tolist()
        t = [[] for _ in fns]
        for _ in range(a.rounds):
            for i, fn in enumerate(fns):
                t[i].append(_timed(fn, a.iters))
        med = [sorted(v)[len(v) // 2] for v in t]
        rng = [f"[{min(v):.1f}, {max(v):.1f}]" for v in t]
        say(f"{b} x {c} x {h}x{w}: {100 * s[0] / (b * h * w):.1f} % of the pixels in view, "
            f"{100 * s[2] / (b * (h - 2) * (w - 2)):.1f} % of the windows")
        say(f"  sums {med[0]:8.1f} us {rng[0]}  grad {med[1]:8.1f} us {rng[1]}  two launches {med[0] + med[1]:8.1f} us")
        say(f"  losses.photometric_loss + backward {med[2]:8.1f} us {rng[2]}")
        say(f"  torch-op composition + backward {med[3]:8.1f} us {rng[3]}  "
            f"composition / two launches {med[3] / (med[0] + med[1]):.2f}  composition / wrapped {med[3] / med[2]:.2f}")
        say(f"  loss hip {lh:.7g} torch {lt:.7g}  |ddisp hip - torch| 99.9th percentile {g999:.3e} max {gdiff:.3e} "
            f"(max |ddisp| {gmax:.3e})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
