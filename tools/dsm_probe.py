#!/usr/bin/env python3
"""The surface model (lea_dsm_splat_f32 / lea_dsm_resolve_f32) at the bench shapes, in one process:

  * the scatter through the C ABI on one stream, buffers allocated once, in both forms (global
    atomics; LDS-staged), on a model-like nadir field (an aerial relief: disparities 40 .. 48 px of
    the tests' slanted recipe, organised points from ``kernels.reproject``, ``row_width`` = the
    image's width, colours, radius 0.5) at 576 x 960 and 2048 x 2048 with cells of 1, 2 and 4 ground
    sample distances (about 1, 4 and 16 points a cell), the same on a grid turned by 30 degrees, and
    the worst case of contention, every row in one cell; and with consecutive runs of rows in
    place of patches (``row_width`` 0, what a cloud's compact rows get); the grid already holds the
    cloud (the steady state of a mosaic: no atomic changes a value), ``lea_dsm_clear`` is timed on
    its own, and clear + splat gives the first add to an empty grid;
  * ``lea_dsm_resolve_f32`` with 0 and 3 fill passes;
  * the same z-buffer at radius 0 from torch ops (projection, mask, ``scatter_reduce`` ``amax`` on
    int64 keys) and on the host (copy, numpy ``maximum.at``, copy), compared with the call's grid;
  * beside them the same run's plain forward (C2), its ``reproject`` call, and the box's
    device-to-device copy bandwidth, against which the bytes the scatter has to move (points and
    colours read once, every hit cell's key read and written once, however many rows cover it: the
    global form moves more) are read.

Warmed up, then ``--rounds`` alternating windows of ``--iters`` calls each, HIP events; medians of
the windows with their range.  The host path runs once.  Writes the lines to ``--out`` as well.

  python tools/dsm_probe.py [--iters 20] [--rounds 5] [--out profiles/dsm_probe.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from leastereo_amd import _lib, dsm, kernels  # noqa: E402
from leastereo_amd.config import LEAStereoArgs, default_arch_args  # noqa: E402
from leastereo_amd.model import LEAStereo  # noqa: E402
from tests import dsm_judge as J  # noqa: E402
from tests import pointcloud_judge as pj  # noqa: E402

SHAPES = [("C2", 576, 960, 192), ("scene", 2048, 2048, None)]  # name, H, W, maxdisp of the forward beside it
D_FAR, D_NEAR = 40.0, 48.0
RADIUS = 0.5


def relief(h, w):
    """The tests' slanted recipe squeezed into D_FAR .. D_NEAR: a relief of a fifth of the flying height."""
    d, e = pj.slanted_field((1, h, w), seed=1)
    with np.errstate(all="ignore"):
        d = (D_FAR + (d - 8.0) * ((D_NEAR - D_FAR) / 52.0)).astype(np.float32)
    return d, e


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def measure(fns, iters, rounds, slow=()):
    for fn in fns:
        fn()
        _timed(fn, 2)
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t[i].append(_timed(fn, max(2, iters // 5) if i in slow else iters))
    return [(sorted(v)[len(v) // 2], min(v), max(v)) for v in t]


def torch_dsm(points, colours, G, gh, gw):
    """The radius-0 z-buffer from torch ops: int64 keys ((ord >> 1) << 32 | colour, so that they stay
    positive), scatter_reduce amax over the nearest cells."""
    p = points.reshape(-1, 3)
    u, v, z = (((G[r, 0] * p[:, 0] + G[r, 1] * p[:, 1]) + G[r, 2] * p[:, 2]) + G[r, 3] for r in range(3))
    ok = torch.isfinite(p).all(1) & torch.isfinite(u) & torch.isfinite(v) & torch.isfinite(z)
    c, r = torch.floor(u + 0.5), torch.floor(v + 0.5)
    ok &= (c >= 0) & (c < gw) & (r >= 0) & (r < gh)
    zero = torch.zeros_like(c)
    idx = torch.where(ok, r, zero).to(torch.int64) * gw + torch.where(ok, c, zero).to(torch.int64)
    bits = z.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    o = torch.where(bits >= 0x80000000, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    col = colours.reshape(-1, 3).to(torch.int64)
    key = ((o >> 1) << 32) | (col[:, 0] << 16) | (col[:, 1] << 8) | col[:, 2]
    key = torch.where(ok, key, torch.zeros_like(key))
    return torch.zeros(gh * gw, device=p.device, dtype=torch.int64).scatter_reduce_(0, idx, key, "amax")


def host_dsm(points, colours, G, gh, gw):
    return J.splat_vec(points.reshape(-1, 3), G, gh, gw, colours=colours.reshape(-1, 3), radius=0.0)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dsm_probe.txt"))
    a = ap.parse_args()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; microseconds, median of {a.rounds} alternating windows of {a.iters} calls "
        f"[min, max]; organised points [H, W, 3] with row_width W, colours, radius {RADIUS} unless said otherwise; the "
        f"grid already holds the cloud")
    src = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    copies = sorted(_timed(lambda: dst.copy_(src), 10) for _ in range(5))
    copy_bw = 2 * src.numel() * 4 / (copies[2] * 1e-6)
    say(f"device-to-device copy of {src.numel() * 4 >> 20} MiB: {copies[2]:.1f} us [{copies[0]:.1f}, {copies[-1]:.1f}] = "
        f"{copy_bw / 1e12:.2f} TB/s read + written (the box's measured copy bandwidth)")
    del src, dst
    verdict = []
    for name, h, w, md in SHAPES:
        n = h * w
        Q = pj.recipe_q(h, w)
        d_h, e_h = relief(h, w)
        disp, excl = torch.from_numpy(d_h).cuda(), torch.from_numpy(e_h).cuda()
        img = torch.from_numpy(pj.recipe_image((1, h, w), seed=3)[..., :3].copy()).cuda()
        cloud = kernels.reproject(disp, Q, img, excl, want_points=True)
        points = cloud.points.contiguous()  # [1, H, W, 3], NaN where not valid
        valid = int(cloud.count[0])
        gsd = float(np.linalg.norm(dsm.grid_from_view(Q, h, w, (D_FAR, D_NEAR))[0][0, :3])) ** -1
        say(f"{name} {h}x{w} ({n} px, {valid} points); ground sample distance at the far disparity {gsd:.6f}")
        a30 = np.deg2rad(30.0)
        turned = np.eye(4)
        turned[:2, :2] = [[np.cos(a30), -np.sin(a30)], [np.sin(a30), np.cos(a30)]]
        setups = []  # (label, G, gh, gw, points, colours, rows, row_width, radius)
        for pose, pname in ((None, "nadir"), (turned, "30 deg")):
            for k in (1, 2, 4):
                G, gh, gw = dsm.grid_from_view(Q, h, w, (D_FAR, D_NEAR), cell=k * gsd, pose=pose)
                setups.append((f"{pname} cell {k} gsd", G, gh, gw, points, img, n, w, RADIUS))
        G1, gh1, gw1 = setups[0][1:4]
        setups.append(("nadir cell 1 gsd, radius 0", G1, gh1, gw1, points, img, n, w, 0.0))
        setups.append(("nadir cell 1 gsd, radius 0, row_width 0", G1, gh1, gw1, points, img, n, 0, 0.0))
        for k in (0, 2):  # consecutive runs of rows in place of patches (a cloud's compact rows), at the default radius
            setups.append((setups[k][0] + ", row_width 0",) + setups[k][1:7] + (0, RADIUS))
        one = torch.zeros((1, n, 3), device="cuda")
        one[..., 2] = torch.rand((1, n), device="cuda")
        setups.append(("one cell, radius 0", J.AXIS_G, gh1, gw1, one, img, n, 0, 0.0))
        for label, G, gh, gw, pts, col, rows, rw, radius in setups:
            g = torch.from_numpy(np.ascontiguousarray(G, dtype=np.float32)).cuda()
            keys = torch.zeros((1, gh, gw), device="cuda", dtype=torch.int64)
            hits = torch.zeros((1, gh, gw), device="cuda", dtype=torch.int32)
            ws = torch.empty(lib.lea_dsm_resolve_workspace_bytes(1, gh, gw) // 8, device="cuda", dtype=torch.int64)
            height = torch.empty((1, gh, gw), device="cuda", dtype=torch.float32)
            rgb = torch.empty((1, gh, gw, 3), device="cuda", dtype=torch.uint8)
            state = torch.empty((1, gh, gw), device="cuda", dtype=torch.uint8)

            def splat(staging, pts=pts, col=col, g=g, rows=rows, rw=rw, radius=radius, gh=gh, gw=gw, keys=keys,
                      hits=hits):
                _lib.check(lib.lea_dsm_splat_f32(pts.data_ptr(), None, col.data_ptr(), g.data_ptr(), 0, 1, rows, rw,
                                                 radius, staging, gh, gw, keys.data_ptr(), hits.data_ptr(), stream),
                           "splat")

            def resolve(passes, gh=gh, gw=gw, keys=keys, hits=hits, ws=ws, height=height, rgb=rgb, state=state):
                _lib.check(lib.lea_dsm_resolve_f32(keys.data_ptr(), hits.data_ptr(), 1, gh, gw, passes, 3,
                                                   float("nan"), ws.data_ptr(), height.data_ptr(), rgb.data_ptr(),
                                                   None, state.data_ptr(), stream), "resolve")

            def clear(gh=gh, gw=gw, keys=keys, hits=hits):
                _lib.check(lib.lea_dsm_clear(keys.data_ptr(), hits.data_ptr(), 1, gh, gw, stream), "clear")

            grids = []
            for staging in (1, 2):
                clear()
                splat(staging)
                grids.append((keys.clone(), hits.clone()))
            same = torch.equal(grids[0][0], grids[1][0]) and torch.equal(grids[0][1], grids[1][1])
            filled = int((keys != 0).sum())
            kept = int(hits.sum())
            nbytes = rows * 15 + filled * 16  # every row read once, every hit cell's key read and written once
            res = measure([lambda: splat(1), lambda: splat(2), lambda: resolve(0), lambda: resolve(3), clear,
                           lambda: (clear(), splat(1)), lambda: (clear(), splat(2))], a.iters, a.rounds)
            splat(1)
            say(f"  {label}: grid {gh}x{gw}, {kept} rows in the grid, {filled} cells hit "
                f"({kept / max(filled, 1):.2f} rows a hit cell); the two forms' bits equal: {same}")
            for (med, lo, hi), what in zip(res, ("splat global", "splat LDS-staged", "resolve, 0 passes",
                                                 "resolve, 3 passes", "clear", "clear + splat global",
                                                 "clear + splat LDS-staged")):
                extra = ""
                if what.startswith("clear +"):
                    extra = f"  the first add to an empty grid: {med - res[4][0]:.1f} us without the clear"
                if what.startswith("splat"):
                    rate = nbytes / (med * 1e-6)
                    extra = (f"  {nbytes / 1e6:.1f} MB = {rate / 1e12:.2f} TB/s, {100.0 * rate / copy_bw:.0f} % of the "
                             f"copy's")
                say(f"    {what:26s} {med:10.1f} us [{lo:.1f}, {hi:.1f}]{extra}")
            say(f"    LDS-staged / global: {res[1][0] / res[0][0]:.3f}")
            if not label.startswith("one cell"):
                verdict.append((name, label, res[0][0], res[1][0]))
        # the comparisons, at radius 0 on the nadir grid of one ground sample distance
        G, gh, gw = G1, gh1, gw1
        g = torch.from_numpy(np.ascontiguousarray(G, dtype=np.float32)).cuda()
        fns = [lambda: torch_dsm(points, img, g, gh, gw), lambda: kernels.reproject(disp, Q, img, excl, want_points=True)]
        labels = ["torch ops (scatter_reduce amax), radius 0", "reproject (points, count, xyz, rgb, index)"]
        slow = ()
        if md is not None:
            model = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=md)), "cuda").cuda().eval()
            left, right = torch.randn(1, 3, h, w, device="cuda"), torch.randn(1, 3, h, w, device="cuda")

            def forward():
                with torch.no_grad():
                    model(left, right)
            fns.append(forward)
            labels.append("forward")
            slow = (2,)
        res = measure(fns, a.iters, a.rounds, slow)
        for (med, lo, hi), what in zip(res, labels):
            say(f"  {what:45s} {med:10.1f} us [{lo:.1f}, {hi:.1f}]")
        if md is not None:
            del model
        s = dsm.Surface(gh, gw, "cuda", batch=1).add(points, g, colours=img, radius=0.0, row_width=w)
        ours = s.keys[0].cpu().numpy().view(np.uint64)
        tk = torch_dsm(points, img, g, gh, gw).reshape(gh, gw).cpu().numpy()
        same_t = np.array_equal(tk != 0, ours != 0) and np.array_equal(tk >> 32, (ours >> np.uint64(33)).astype(np.int64))
        torch.cuda.synchronize()
        t0 = time.time()
        ph, ch = points.cpu().numpy(), img.cpu().numpy()
        t1 = time.time()
        hk = host_dsm(ph, ch, G, gh, gw)
        t2 = time.time()
        torch.from_numpy(hk.view(np.int64)).cuda()
        torch.cuda.synchronize()
        t3 = time.time()
        say(f"  host path (numpy maximum.at, radius 0): copy out {1e3 * (t1 - t0):.1f} ms, project + scatter "
            f"{1e3 * (t2 - t1):.1f} ms, copy in {1e3 * (t3 - t2):.1f} ms; the call's grid equals the host's: "
            f"{np.array_equal(hk, ours)}; torch's cells and heights (all but the last bit of ord) equal the call's: "
            f"{same_t}")
    say("LDS-staged / global on the model-like fields: " + ", ".join(
        f"{n} {lab} {lds / glob:.2f}" for n, lab, glob, lds in verdict))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
