#!/usr/bin/env python3
"""Rectification (lea_rectify_pair_u8) at the bench shapes, in one process:

  * the call through the C ABI on one stream, buffers allocated once, a uint8 RGB pair rectified
    to its own size with the validity map: from a calibration with the pinhole rational model,
    from one with the fisheye model, and from given maps (``maps_in``); each with the 128 x 8
    workgroup tile and with the 1024 x 1 one (lea_rectify_set_tile);
  * the bytes the call has to move (every source byte once, every output byte, the validity
    map, the given maps) over its time, beside the bandwidth of a device-to-device copy measured
    in the same run;
  * the same images from torch ops: ``grid_sample`` on float copies of the two images with the
    maps already on the device, then round and convert back;
  * the host path the call replaces: device-to-host copy of both images, the bilinear remap on
    the host (``scipy.ndimage.map_coordinates`` where scipy is present, else the numpy judge),
    host-to-device copy of the result;
  * beside them the same run's plain forward (C2, C5).

Warmed up, then ``--rounds`` alternating windows of ``--iters`` calls each, HIP events; medians
of the windows with their range.  The host path runs once per shape.  Writes the lines to
``--out`` as well.

  python tools/rectify_probe.py [--iters 20] [--rounds 5] [--out profiles/rectify_probe.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from leastereo_amd import _lib, kernels  # noqa: E402
from leastereo_amd import rectify as rc  # noqa: E402
from leastereo_amd.config import LEAStereoArgs, default_arch_args  # noqa: E402
from leastereo_amd.model import LEAStereo  # noqa: E402
from tests import rectify_judge as rj  # noqa: E402

# (name, H, W, maxdisp of the forward beside it or None)
SHAPES = [("C2", 576, 960, 192), ("C5", 1008, 1512, 264), ("scene", 2048, 2048, None)]
PS = 3


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def torch_remap(left, right, grid):
    """The pair from torch ops: float copies, grid_sample (bilinear, zeros outside), round, uint8."""
    out = []
    for k, img in enumerate((left, right)):
        x = img.permute(2, 0, 1).unsqueeze(0).float()
        y = torch.nn.functional.grid_sample(x, grid[k:k + 1], mode="bilinear", padding_mode="zeros", align_corners=True)
        out.append(torch.round(y)[0].permute(1, 2, 0).to(torch.uint8))
    return out


def host_remap(img, sx, sy):
    try:
        from scipy.ndimage import map_coordinates
        out = np.stack([map_coordinates(img[..., c], [sy, sx], order=1, mode="constant", cval=0.0, output=np.float32)
                        for c in range(img.shape[-1])], -1)
        return np.rint(out).astype(np.uint8), "scipy.ndimage.map_coordinates"
    except ImportError:
        return rj.pixel32(img, sx, sy, 0)[0], "numpy judge"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rectify_probe.txt"))
    a = ap.parse_args()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; microseconds, median of {a.rounds} alternating windows of {a.iters} calls "
        f"[min, max]; one uint8 RGB pair (B = 1, pix_stride {PS}) rectified to its own size, fill 0, with the validity "
        f"map, without maps_out")
    src = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    copies = sorted(_timed(lambda: dst.copy_(src), 10) for _ in range(5))
    copy_bw = 2 * src.numel() * 4 / (copies[2] * 1e-6)
    say(f"device-to-device copy of {src.numel() * 4 >> 20} MiB: {copies[2]:.1f} us [{copies[0]:.1f}, {copies[-1]:.1f}] = "
        f"{copy_bw / 1e12:.2f} TB/s read + written (the box's measured copy bandwidth)")
    del src, dst
    for name, h, w, md in SHAPES:
        n = h * w
        img = rj.recipe_image((2, h, w), PS, seed=3)
        left, right = torch.from_numpy(img[0]).cuda(), torch.from_numpy(img[1]).cuda()
        calibs = {}
        for rig in ("rational8", "fisheye"):
            cl, cr, R, T = rj.recipe_rig(rig, (h, w))
            calibs[rig] = torch.from_numpy(rc.stereo_rectify(cl, cr, R, T, (h, w)).calib()).cuda()
        maps = kernels.rectify_u8(left, right, calib=calibs["rational8"], want_maps=True).maps.unsqueeze(0).contiguous()
        ol = torch.empty((1, h, w, PS), device="cuda", dtype=torch.uint8)
        orr = torch.empty_like(ol)
        valid = torch.empty((1, 2, h, w), device="cuda", dtype=torch.uint8)

        def call(calib, m):
            _lib.check(lib.lea_rectify_pair_u8(
                left.data_ptr(), right.data_ptr(), PS, 1, h, w, None if calib is None else calib.data_ptr(),
                0 if calib is None else 1, None if m is None else m.data_ptr(), 0 if m is None else 1, h, w, 0,
                ol.data_ptr(), orr.data_ptr(), valid.data_ptr(), None, stream), "rectify")

        def tiled(tile, calib, m):
            lib.lea_rectify_set_tile(tile)
            call(calib, m)
            lib.lea_rectify_set_tile(0)

        variants = [("calib, pinhole rational", calibs["rational8"], None), ("calib, fisheye", calibs["fisheye"], None),
                    ("maps_in", None, maps)]
        fns, names, nbytes = [], [], []
        for tile, tname in ((0, "128x8"), (1, "1024x1")):
            for vname, c, m in variants:
                fns.append(lambda tile=tile, c=c, m=m: tiled(tile, c, m))
                names.append(f"{vname}, tile {tname}")
                nbytes.append(2 * n * (PS + PS + 1 + (8 if m is not None else 0)))
        ncall = len(fns)
        gx = maps[0, :, 0] / (w - 1) * 2 - 1
        gy = maps[0, :, 1] / (h - 1) * 2 - 1
        grid = torch.stack([gx, gy], -1).contiguous()
        fns.append(lambda: torch_remap(left, right, grid))
        names.append("torch ops (float copies, grid_sample, round)")
        if md is not None:
            model = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=md)), "cuda").cuda().eval()
            fl, fr = torch.randn(1, 3, h, w, device="cuda"), torch.randn(1, 3, h, w, device="cuda")

            def forward():
                with torch.no_grad():
                    model(fl, fr)
            fns.append(forward)
            names.append("forward")
        for fn in fns:
            fn()
            _timed(fn, 3)
        t = [[] for _ in fns]
        for _ in range(a.rounds):
            for i, fn in enumerate(fns):
                t[i].append(_timed(fn, a.iters if names[i] != "forward" else max(2, a.iters // 5)))
        med = [sorted(v)[len(v) // 2] for v in t]
        call(calibs["rational8"], None)
        torch.cuda.synchronize()
        share = float(valid.float().mean())
        say(f"{name} {h}x{w} ({n} px a view; {100 * share:.1f} % of the rectified pixels have a source under the pinhole "
            f"rig):")
        for i, lab in enumerate(names):
            extra = ""
            if i < ncall:
                rate = nbytes[i] / (med[i] * 1e-6)
                extra = (f"  {nbytes[i] / 1e6:.1f} MB = {rate / 1e12:.2f} TB/s, {100.0 * rate / copy_bw:.0f} % of the "
                         f"copy's")
            say(f"  {lab:46s} {med[i]:10.1f} us [{min(t[i]):.1f}, {max(t[i]):.1f}]{extra}")
        say(f"  torch ops / call (pinhole, 128x8): {med[ncall] / med[0]:.1f}")
        if md is not None:
            say(f"  call (pinhole, 128x8) / forward: {med[0] / med[names.index('forward')]:.5f}")
            del model
        # the torch composition against the call, and the host path
        tl, _ = torch_remap(left, right, grid)
        diff = (tl.int() - ol[0].int()).abs()
        say(f"  torch ops vs the call, left view: {100.0 * float((diff > 0).float().mean()):.2f} % of the bytes differ, "
            f"largest difference {int(diff.max())} (grid_sample normalises the coordinates and blends partly outside "
            f"taps with zeros: it is not the same definition)")
        mh = maps[0].cpu().numpy()
        t0 = time.time()
        lh, rh = left.cpu().numpy(), right.cpu().numpy()
        t1 = time.time()
        hl, how = host_remap(lh, mh[0, 0], mh[0, 1])
        hr, _ = host_remap(rh, mh[1, 0], mh[1, 1])
        t2 = time.time()
        torch.from_numpy(hl).cuda(), torch.from_numpy(hr).cuda()
        torch.cuda.synchronize()
        t3 = time.time()
        say(f"  host path ({how}, maps already made): copy out {1e3 * (t1 - t0):.1f} ms, remap of both views "
            f"{1e3 * (t2 - t1):.1f} ms, copy in {1e3 * (t3 - t2):.1f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
