#!/usr/bin/env python3
"""The edge-aware loss at the training shapes (4 x 288x576, 1 x 576x960), in one process:

  * the three launches (lea_median5x5_f32 twice over, lea_edge_loss_f32,
    lea_edge_loss_grad_f32) through the C ABI on one stream, and the whole
    ``losses.combined_loss(...).backward()`` that wraps them;
  * the same loss composed from torch ops (masked smooth_l1, F.conv2d Sobels, exp, mean;
    forward and backward), fed the device median;
  * the device -> host -> twice-median -> device round trip that the reference's design
    implies every step (edge_detection.py:7-11,69); cv2 is not available, scipy's
    median_filter stands in for it (wall clock, ``--host-reps`` repetitions).

Warmed up, then ``--rounds`` alternating windows of ``--iters`` calls each, HIP events;
medians of the windows with their range.  Writes the lines to ``--out`` as well.

  python tools/loss_probe.py [--iters 20] [--rounds 9] [--out profiles/loss_probe.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leastereo_amd import _lib, kernels, losses  # noqa: E402

SHAPES = [(4, 288, 576), (1, 576, 960)]
MAXDISP, W_EDGE = 192.0, 0.2


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def torch_loss(pred, target, tsmooth):
    mask = (target < MAXDISP) & (target > 0.001)
    direct = F.smooth_l1_loss(pred[mask], target[mask], reduction="mean")
    kx = pred.new_tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]).view(1, 1, 3, 3)
    ky = pred.new_tensor([[1, 2, 1], [0, 0, 0], [-1, -2, -1]]).view(1, 1, 3, 3)
    ox, oy = F.conv2d(pred.unsqueeze(1), kx), F.conv2d(pred.unsqueeze(1), ky)
    tx, ty = F.conv2d(tsmooth.unsqueeze(1), kx), F.conv2d(tsmooth.unsqueeze(1), ky)
    return direct + W_EDGE * torch.mean(torch.abs(ox) * torch.exp(-torch.abs(tx)) +
                                        torch.abs(oy) * torch.exp(-torch.abs(ty)))


def host_round_trip(target):
    from scipy import ndimage
    t = target.cpu().numpy()
    sm = np.stack([ndimage.median_filter(ndimage.median_filter(i, size=5, mode="nearest"), size=5, mode="nearest")
                   for i in t])
    return torch.from_numpy(sm).to(target.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "loss_probe.txt"))
    a = ap.parse_args()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; microseconds, median of {a.rounds} alternating windows of {a.iters} "
        f"calls [min, max]; maxdisp {MAXDISP:g}, edge weight {W_EDGE}")
    for b, h, w in SHAPES:
        target = torch.rand(b, h, w, device="cuda", generator=g) * (MAXDISP + 8)
        target[:, : h // 4, : w // 4] = 0
        pred = target + 1.5 * torch.randn(b, h, w, device="cuda", generator=g)
        ts, dpred = torch.empty_like(target), torch.empty_like(target)
        sums = torch.empty(4, device="cuda", dtype=torch.float64)
        ws = torch.empty(lib.lea_edge_loss_workspace_bytes(b, h, w) // 8, device="cuda", dtype=torch.float64)
        scales = torch.tensor([1.0, W_EDGE], device="cuda")
        hw = h * w
        ptr = [t.data_ptr() for t in (pred, target, ts)]

        def median():
            _lib.check(lib.lea_median5x5_f32(ptr[1], hw, ptr[2], hw, b, h, w, 2, stream), "median")

        def fwd():
            _lib.check(lib.lea_edge_loss_f32(ptr[0], hw, ptr[1], hw, ptr[2], hw, b, h, w, MAXDISP, sums.data_ptr(),
                                             ws.data_ptr(), stream), "sums")

        def bwd():
            _lib.check(lib.lea_edge_loss_grad_f32(ptr[0], hw, ptr[1], hw, ptr[2], hw, sums.data_ptr(),
                                                  scales.data_ptr(), dpred.data_ptr(), hw, b, h, w, MAXDISP, stream),
                       "grad")

        p_hip = pred.clone().requires_grad_()
        p_torch = pred.clone().requires_grad_()

        def wrapped():
            p_hip.grad = None
            losses.combined_loss(p_hip, target, MAXDISP, W_EDGE).backward()

        def composed():
            p_torch.grad = None
            torch_loss(p_torch, target, ts).backward()

        fns = (median, fwd, bwd, wrapped, composed)
        for fn in fns:
            fn()
            _timed(fn, a.iters)
        # the two forms agree (the composition sums in f32)
        lh = float(losses.combined_loss(pred, target, MAXDISP, W_EDGE))
        lt = float(torch_loss(pred, target, ts))
        gdiff = float((p_hip.grad - p_torch.grad).abs().max())
        t = [[] for _ in fns]
        for _ in range(a.rounds):
            for i, fn in enumerate(fns):
                t[i].append(_timed(fn, a.iters))
        med = [sorted(v)[len(v) // 2] for v in t]
        host = []
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sm = host_round_trip(target)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e6)
        same = bool(torch.equal(sm, ts))
        rng = [f"[{min(v):.1f}, {max(v):.1f}]" for v in t]
        say(f"{b} x {h}x{w}")
        say(f"  median x2 {med[0]:8.1f} us {rng[0]}  sums {med[1]:8.1f} us {rng[1]}  grad {med[2]:8.1f} us {rng[2]}  "
            f"three launches {med[0] + med[1] + med[2]:8.1f} us")
        say(f"  losses.combined_loss + backward {med[3]:8.1f} us {rng[3]}")
        say(f"  torch-op composition + backward (device median given) {med[4]:8.1f} us {rng[4]}  "
            f"composition / three launches {med[4] / (med[0] + med[1] + med[2]):.2f}  "
            f"composition / wrapped {med[4] / med[3]:.2f}")
        say(f"  host round trip, scipy twice-median {sorted(host)[len(host) // 2]:10.0f} us "
            f"[{min(host):.0f}, {max(host):.0f}]  same bits as the device median: {same}")
        say(f"  loss hip {lh:.7g} torch {lt:.7g}  max |dpred hip - torch| {gdiff:.3e}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
