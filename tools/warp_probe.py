#!/usr/bin/env python3
"""The forward warp (lea_forward_warp_f32) at the bench shapes, in one process:

  * the call through the C ABI on one stream, buffers allocated once, C = 3, all four outputs,
    fill on, on the model-like field of the other probes, at s = 0.3 and s = 1.0;
  * the bytes the call has to move -- (C + 1) planes and the exclude bytes in, the requested
    planes out -- over its time, beside the bandwidth of a device-to-device copy measured in the
    same run;
  * a point splat from torch ops (``scatter_reduce`` ``amax`` on packed int64 keys of
    (orderable disparity bits, column), then a gather).  It is NOT the same output: whole-pixel
    targets, no segments, so slanted surfaces crack at s > 1, no interpolation, no fill.  It is
    the lower-quality result a user gets without the kernel, timed as the nearest thing torch has;
  * the host path: device-to-host copy, the same point splat in vectorised numpy, host-to-device copy;
  * beside them the same run's plain forward at C2 and C5 and, once per run, the whole-model
    train step of tools/train_bench.py at its default shape (288 x 576, maxdisp 96).

Warmed up, then ``--rounds`` alternating windows of ``--iters`` calls each, HIP events; medians
of the windows with their range.  The host path runs once per case.  Writes the lines to
``--out`` as well.

  python tools/warp_probe.py [--iters 20] [--rounds 5] [--out profiles/warp_probe.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from leastereo_amd import _lib  # noqa: E402
from leastereo_amd.config import LEAStereoArgs, default_arch_args  # noqa: E402
from leastereo_amd.model import LEAStereo  # noqa: E402
from tests import pointcloud_judge as pj  # noqa: E402

# (name, B, H, W, maxdisp of the forward beside it or None)
SHAPES = [("C2", 1, 576, 960, 192), ("C5", 1, 1008, 1512, 264), ("scene", 1, 2048, 2048, None)]
SCALES = (0.3, 1.0)
C = 3


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def torch_splat(img, d, e, s):
    """Nearest-surface point splat from torch ops: image [C, H, W], d / e [H, W] -> (view, hit)."""
    c, h, w = img.shape
    x = torch.arange(w, device=d.device, dtype=torch.float32)[None, :]
    u = torch.round(x - s * d)
    ok = torch.isfinite(d) & (e == 0) & (u >= 0) & (u <= w - 1)
    bits = d.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    order = torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)
    key = (order << 31) | torch.arange(w, device=d.device, dtype=torch.int64)[None, :]
    tgt = torch.where(ok, u, torch.zeros_like(u)).to(torch.int64) + torch.arange(h, device=d.device)[:, None] * w
    best = torch.full((h * w,), -1, device=d.device, dtype=torch.int64)
    best.scatter_reduce_(0, tgt[ok], key[ok], "amax", include_self=True)
    hit = best >= 0
    src = (best & 0x7FFFFFFF).clamp_(0, w - 1) + torch.arange(h, device=d.device).repeat_interleave(w) * w
    view = img.reshape(c, -1)[:, src] * hit
    return view.reshape(c, h, w), hit.reshape(h, w)


def host_splat(img, d, e, s):
    """The same splat in vectorised numpy: per row-major target the candidate of the largest disparity."""
    c, h, w = img.shape
    with np.errstate(all="ignore"):
        u = np.rint(np.arange(w, dtype=np.float32)[None, :] - np.float32(s) * d)
        ok = np.isfinite(d) & (e == 0) & (u >= 0) & (u <= w - 1)
    ys, xs = np.nonzero(ok)
    tgt = ys * w + u[ok].astype(np.int64)
    order = np.lexsort((xs, d[ok], tgt))  # by target, then disparity, then column: the last of a target wins
    tgt_s = tgt[order]
    last = np.r_[tgt_s[1:] != tgt_s[:-1], True]
    view = np.zeros((c, h * w), np.float32)
    view[:, tgt_s[last]] = img.reshape(c, -1)[:, (ys * w + xs)[order][last]]
    return view.reshape(c, h, w)


def train_step_ms(steps=3, warmup=2):
    import torch.nn.functional as F
    model = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=96)), "cuda").cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-4, momentum=0.9)
    left = torch.randn(1, 3, 288, 576, device="cuda").requires_grad_(True)
    right = torch.randn(1, 3, 288, 576, device="cuda").requires_grad_(True)
    target = torch.rand(1, 288, 576, device="cuda") * 95

    def step():
        opt.zero_grad()
        F.smooth_l1_loss(model(left, right), target).backward()
        opt.step()
    for _ in range(warmup):
        step()
    return _timed(step, steps) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "warp_probe.txt"))
    a = ap.parse_args()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; microseconds, median of {a.rounds} alternating windows of {a.iters} "
        f"calls [min, max]; C = {C}, max_diff 1, max_stretch 4, fill on, outputs warped + zview + state + source")
    src = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    copies = sorted(_timed(lambda: dst.copy_(src), 10) for _ in range(5))
    copy_bw = 2 * src.numel() * 4 / (copies[2] * 1e-6)
    say(f"device-to-device copy of {src.numel() * 4 >> 20} MiB: {copies[2]:.1f} us [{copies[0]:.1f}, {copies[-1]:.1f}] = "
        f"{copy_bw / 1e12:.2f} TB/s read + written (the box's measured copy bandwidth)")
    del src, dst
    say(f"whole-model train step, 288x576, maxdisp 96 (tools/train_bench.py --whole 1): {train_step_ms():.1f} ms")
    for name, b, h, w, md in SHAPES:
        n = b * h * w
        d_h, e_h = pj.slanted_field((b, h, w), seed=1)
        e_h = e_h.astype(np.uint8)
        img_h = np.random.default_rng(3).standard_normal((b, C, h, w)).astype(np.float32)
        img, d, e = torch.from_numpy(img_h).cuda(), torch.from_numpy(d_h).cuda(), torch.from_numpy(e_h).cuda()
        scales = {s: torch.full((b,), s, device="cuda") for s in SCALES}
        warped = torch.empty((b, C, h, w), device="cuda")
        zview, source = torch.empty((b, h, w), device="cuda"), torch.empty((b, h, w), device="cuda")
        state = torch.empty((b, h, w), device="cuda", dtype=torch.uint8)

        def call(s):
            _lib.check(lib.lea_forward_warp_f32(
                img.data_ptr(), C * h * w, d.data_ptr(), h * w, e.data_ptr(), scales[s].data_ptr(), b, C, h, w, 1.0, 4.0,
                1, 0.0, warped.data_ptr(), zview.data_ptr(), state.data_ptr(), source.data_ptr(), stream), "forward_warp")

        fns = [lambda s=s: call(s) for s in SCALES] + [lambda s=s: torch_splat(img[0], d[0], e[0], s) for s in SCALES]
        names = [f"call, s = {s}" for s in SCALES] + [f"torch-ops point splat (not the same output), s = {s}"
                                                      for s in SCALES]
        if md is not None:
            model = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=md)), "cuda").cuda().eval()
            right = torch.randn(b, 3, h, w, device="cuda")

            def forward():
                with torch.no_grad():
                    model(img, right)
            fns.append(forward)
            names.append("forward")
        for fn in fns:
            fn()
            _timed(fn, 2)
        t = [[] for _ in fns]
        for _ in range(a.rounds):
            for i, fn in enumerate(fns):
                t[i].append(_timed(fn, a.iters if names[i] != "forward" else max(2, a.iters // 5)))
        med = [sorted(v)[len(v) // 2] for v in t]
        nbytes = n * (4 * (C + 1) + 1) + n * (4 * C + 4 + 1 + 4)
        say(f"{name} B={b} {h}x{w} ({n} px), {100.0 * float(np.isfinite(d_h).mean()):.1f} % finite, "
            f"{100.0 * float((e_h != 0).mean()):.1f} % excluded, disparities {np.nanmin(d_h):.1f} .. {np.nanmax(d_h):.1f}:")
        for i, lab in enumerate(names):
            extra = ""
            if i < len(SCALES):
                call(SCALES[i])
                torch.cuda.synchronize()
                rate = nbytes / (med[i] * 1e-6)
                extra = (f"  {100.0 * float((state != 0).float().mean()):.2f} % holes, {nbytes / 1e6:.1f} MB = "
                         f"{rate / 1e12:.2f} TB/s, {100.0 * rate / copy_bw:.0f} % of the copy's")
            say(f"  {lab:52s} {med[i]:10.1f} us [{min(t[i]):.1f}, {max(t[i]):.1f}]{extra}")
        say("  torch-ops splat / call: " + ", ".join(f"s = {s}: {med[len(SCALES) + i] / med[i]:.1f}"
                                                     for i, s in enumerate(SCALES)))
        if md is not None:
            fw = med[names.index("forward")]
            say("  call / forward: " + ", ".join(f"s = {s}: {med[i] / fw:.5f}" for i, s in enumerate(SCALES)))
            del model
        for s in SCALES:
            t0 = time.time()
            ih, dh, eh = img.cpu().numpy(), d.cpu().numpy(), e.cpu().numpy()
            t1 = time.time()
            hv = host_splat(ih[0], dh[0], eh[0], s)
            t2 = time.time()
            torch.from_numpy(hv).cuda()
            torch.cuda.synchronize()
            t3 = time.time()
            tv, th = torch_splat(img[0], d[0], e[0], s)
            same = bool(np.array_equal(tv.cpu().numpy(), hv))
            say(f"  host path, s = {s} (numpy point splat): copy out {1e3 * (t1 - t0):.1f} ms, splat {1e3 * (t2 - t1):.1f} ms, "
                f"copy in {1e3 * (t3 - t2):.1f} ms; equal to the torch-ops splat: {same}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
