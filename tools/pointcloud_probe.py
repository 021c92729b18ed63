#!/usr/bin/env python3
"""The point cloud (lea_disparity_pointcloud_f32) at the bench shapes, in one process:

  * the call through the C ABI on one stream, buffers allocated once, on three fields: the
    model-like recipe of the tests with more pixels excluded (about 90 % valid), an all-valid
    field and a field with 1 % of its pixels valid; two variants each: ``plain`` (count, xyz,
    index) and ``full`` (also rgb from a uint8 image and the normals); the per-kernel device
    times of one call from torch's profiler;
  * the bytes the call has to move (computed from the shape, the variant and the count) over
    its time, beside the bandwidth of a device-to-device copy measured in the same run;
  * the same compact result from torch ops (mask, ``torch.nonzero``, gathers: the nonzero
    synchronises the host), compared with the call's count and indices;
  * the host path that the call replaces: device-to-host copy of the maps, the reprojection
    and the boolean mask in numpy, host-to-device copy of the points;
  * beside them the same run's plain forward (C2, C5) and the same run's ``fgs_refine`` call
    (T = 3) at the same size, the yardsticks.

Warmed up, then ``--rounds`` alternating windows of ``--iters`` calls each, HIP events; medians
of the windows with their range.  The host path runs once per field.  Writes the lines to
``--out`` as well.

  python tools/pointcloud_probe.py [--iters 20] [--rounds 5] [--out profiles/pointcloud_probe.txt]
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
from leastereo_amd.config import LEAStereoArgs, default_arch_args  # noqa: E402
from leastereo_amd.model import LEAStereo  # noqa: E402
from tests import pointcloud_judge as pj  # noqa: E402

# (name, B, H, W, maxdisp of the forward beside it or None)
SHAPES = [("C2", 1, 576, 960, 192), ("C5", 1, 1008, 1512, 264), ("scene", 1, 2048, 2048, None)]


def fields(b, h, w):
    """(name, disp [B, H, W], exclude)"""
    d, e = pj.slanted_field((b, h, w), seed=1)
    rng = np.random.default_rng(2)
    yield "model-like", d, np.where(rng.random(d.shape) < 0.05, 1, e).astype(np.uint8)
    clean = np.where(np.isfinite(d) & (d > 0), d, np.float32(20.0)).astype(np.float32)
    yield "all valid", clean, np.zeros(d.shape, np.uint8)
    yield "1 % valid", clean, (rng.random(d.shape) >= 0.01).astype(np.uint8)


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def kernel_times(fn):
    """Mean device microseconds per kernel name of one call, from torch's profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            if "pc_" in ev.key:
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = ev.cuda_time_total
                out[ev.key.split("(")[0].split("::")[-1]] = (total / ev.count, ev.count // 5)
        return out
    except Exception as e:  # the profiler is an extra: the event timings stand without it
        return {"profiler unavailable": (float("nan"), repr(e)[:80])}


def call_bytes(n, count, full, pix):
    """The bytes the three launches have to move: disp and exclude read by the count and by the
    scatter launch, the block counts written, read, rewritten and read, a valid pixel's row
    written, and with ``full`` its colour read and its four neighbours' disparity and exclude
    (counted once each: a neighbour is another lane's own pixel and comes from the cache)."""
    b = 2 * n * 5 + 4 * 4 * (-(-n // 1024)) + count * (12 + 4)
    if full:
        b += count * (pix + 3 + 12)
    return b


def torch_cloud(d, e, img, q, w, full):
    """The compact result from torch ops: the mask, torch.nonzero (a host synchronisation: the
    size of its result goes to the host), the gathers and the reprojection of the kept pixels."""
    flat = d.reshape(-1)
    ok = torch.isfinite(flat) & (flat > 0) & (e.reshape(-1) == 0)
    idx = torch.nonzero(ok).squeeze(1)
    dd = flat[idx]
    x = (idx % w).to(torch.float32)
    y = torch.div(idx, w, rounding_mode="floor").to(torch.float32)
    h = [((q[r, 0] * x + q[r, 1] * y) + q[r, 2] * dd) + q[r, 3] for r in range(4)]
    xyz = torch.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], 1)
    rgb = img.reshape(-1, img.shape[-1])[idx, :3] if full else None
    return idx, xyz, rgb


def host_cloud(d, e, img, q, full):
    """What a user does on the host today: reprojectImageTo3D restated in numpy, then a boolean mask."""
    h, w = d.shape[-2:]
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    with np.errstate(all="ignore"):
        hh = [q[r, 0] * x + q[r, 1] * y + q[r, 2] * d[0] + q[r, 3] for r in range(4)]
        pts = np.stack([hh[0] / hh[3], hh[1] / hh[3], hh[2] / hh[3]], -1)
        ok = np.isfinite(d[0]) & (d[0] > 0) & (e[0] == 0) & np.isfinite(pts).all(-1)
    return pts[ok], (img[0][ok][:, :3] if full else None), np.flatnonzero(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pointcloud_probe.txt"))
    a = ap.parse_args()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; microseconds, median of {a.rounds} alternating windows of {a.iters} "
        f"calls [min, max]; min_disp 0, normal_max_diff 1, capacity H*W; plain = count, xyz, index; full = plain + "
        f"rgb (uint8 RGB image) + normals")
    src = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    copies = sorted(_timed(lambda: dst.copy_(src), 10) for _ in range(5))
    copy_bw = 2 * src.numel() * 4 / (copies[2] * 1e-6)
    say(f"device-to-device copy of {src.numel() * 4 >> 20} MiB: {copies[2]:.1f} us [{copies[0]:.1f}, {copies[-1]:.1f}] = "
        f"{copy_bw / 1e12:.2f} TB/s read + written (the box's measured copy bandwidth)")
    del src, dst
    for name, b, h, w, md in SHAPES:
        n = b * h * w
        Q = pj.recipe_q(h, w)
        q32 = Q.astype(np.float32)
        q = torch.from_numpy(q32).cuda()
        ws = torch.empty(lib.lea_disparity_pointcloud_workspace_bytes(b, h, w) // 4, device="cuda", dtype=torch.int32)
        count = torch.empty((b,), device="cuda", dtype=torch.int32)
        xyz = torch.empty((b, n // b, 3), device="cuda", dtype=torch.float32)
        nrm = torch.empty_like(xyz)
        rgb = torch.empty((b, n // b, 3), device="cuda", dtype=torch.uint8)
        index = torch.empty((b, n // b), device="cuda", dtype=torch.int32)
        img_h = pj.recipe_image((b, h, w), seed=3)[..., :3].copy()
        img = torch.from_numpy(img_h).cuda()
        cases = [(fname, torch.from_numpy(d).cuda(), torch.from_numpy(e).cuda()) for fname, d, e in fields(b, h, w)]

        def call(case, full):
            _, dd, ee = case
            _lib.check(lib.lea_disparity_pointcloud_f32(
                dd.data_ptr(), ee.data_ptr(), img.data_ptr() if full else None, 3 if full else 0, q.data_ptr(), 0, b, h,
                w, 0.0, float("inf"), 1.0, n // b, ws.data_ptr(), None, None, count.data_ptr(), xyz.data_ptr(),
                rgb.data_ptr() if full else None, index.data_ptr(), nrm.data_ptr() if full else None, stream),
                "pointcloud")

        fns, names = [], []
        for c in cases:
            for full in (False, True):
                fns.append(lambda c=c, full=full: call(c, full))
                names.append(f"{c[0]} {'full' if full else 'plain'}")
        ncall = len(fns)
        for c in cases:
            for full in (False, True):
                fns.append(lambda c=c, full=full: torch_cloud(c[1], c[2], img, q, w, full))
                names.append(f"torch ops, {c[0]} {'full (no normals)' if full else 'plain'}")
        guide = torch.randn(b, 3, h, w, device="cuda")
        conf = torch.rand(b, h, w, device="cuda")
        fns.append(lambda: kernels.fgs_refine(guide, cases[0][1], conf, cases[0][2]))
        names.append("fgs_refine")
        if md is not None:
            model = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=md)), "cuda").cuda().eval()
            right = torch.randn(b, 3, h, w, device="cuda")

            def forward():
                with torch.no_grad():
                    model(guide, right)
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
        say(f"{name} B={b} {h}x{w} ({n} px):")
        counts = {}
        for c in cases:
            call(c, False)
            counts[c[0]] = int(count.sum())
        for i, lab in enumerate(names):
            extra = ""
            if i < ncall:
                cnt = counts[cases[i // 2][0]]
                nbytes = call_bytes(n, cnt, bool(i % 2), 3)
                rate = nbytes / (med[i] * 1e-6)
                extra = (f"  {cnt} points ({100.0 * cnt / n:.1f} %), {nbytes / 1e6:.1f} MB = {rate / 1e12:.2f} TB/s, "
                         f"{100.0 * rate / copy_bw:.0f} % of the copy's")
            say(f"  {lab:42s} {med[i]:10.1f} us [{min(t[i]):.1f}, {max(t[i]):.1f}]{extra}")
        ref = med[names.index("fgs_refine")]
        say("  call / fgs_refine: " + ", ".join(f"{names[i]} {med[i] / ref:.3f}" for i in range(ncall)))
        say("  torch ops / call: " + ", ".join(f"{names[i]} {med[ncall + i] / med[i]:.1f}" for i in range(ncall)))
        if md is not None:
            fw = med[names.index("forward")]
            say(f"  model-like call / forward: plain {med[0] / fw:.5f}, full {med[1] / fw:.5f}")
            del model
        for c in cases:
            for full in (False, True):
                for k, (us, cnt) in sorted(kernel_times(lambda: call(c, full)).items()):
                    say(f"  {c[0]:10s} {'full' if full else 'plain':5s} kernel {k}: {us:8.1f} us mean, {cnt} launch per call")
        for c in cases:
            fname, dd, ee = c
            call(c, True)
            torch.cuda.synchronize()
            got_n = int(count[0])
            got_idx = index[0, :got_n].cpu().numpy()
            got_xyz = xyz[0, :got_n].cpu().numpy()
            tidx, txyz, _ = torch_cloud(dd, ee, img, q, w, True)
            same_t = got_n == tidx.numel() and np.array_equal(got_idx, tidx.cpu().numpy())
            t0 = time.time()
            dh, eh, ih = dd.cpu().numpy(), ee.cpu().numpy(), img.cpu().numpy()
            t1 = time.time()
            hx, hc, hi = host_cloud(dh, eh, ih, q32, True)
            t2 = time.time()
            torch.from_numpy(hx).cuda(), torch.from_numpy(np.ascontiguousarray(hc)).cuda()
            torch.cuda.synchronize()
            t3 = time.time()
            same_h = got_n == len(hi) and np.array_equal(got_idx, hi)
            err = float(np.abs(got_xyz - hx).max() / np.abs(hx).max()) if same_h and got_n else float("nan")
            say(f"  {fname:10s} host path (numpy, full without normals): copy out {1e3 * (t1 - t0):.1f} ms, reproject + "
                f"mask {1e3 * (t2 - t1):.1f} ms, copy in {1e3 * (t3 - t2):.1f} ms; the call's indices equal torch's: "
                f"{same_t}, the host's: {same_h}; largest |xyz - host| / largest coordinate {err:.1e}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
