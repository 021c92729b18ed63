#!/usr/bin/env python3
"""The training batch transform at the training shape (B = 4, 540x960x3 -> 384x576, shift 0 and
shift 3), in one process:

  (a) the launches of lea_train_transform_u8 alone (the one-workgroup clear, statistics, crop),
      inputs resident on the device, through the C ABI on one stream; also the entry at a 4x4
      crop, which is the clear and the statistics launch with next to no crop work;
  (b) the host-to-device copy of the decoded uint8 pairs, the disparity and the params (pinned
      host memory), then the launches: what a loader that hands over decoded samples pays;
  (c) the reference's host path: the numpy judge's set_rgb_layers + train_transform
      (tests/transform_judge.py, the reference's expressions) per sample on one core of this
      box, then the copy of the float32 crops (pinned) to the device.

(a) and (b) are HIP-event timed: a warm-up, then ``--reps`` windows of ``--iters`` calls, the
median window with its range; (c) is wall clock around a device synchronise, ``--host-reps``
repetitions.  Bytes of (a) are the algorithmic ones (each source byte once per pass that needs
it, each output byte once); the copy figure beside it is tools/bw_probe.py's, run as a child
process first.  Writes the lines to ``--out`` as well.

  python tools/transform_probe.py [--reps 20] [--iters 20] [--out profiles/transform_probe.txt]
"""
import argparse
import os
import random
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, H, W, PS, CH, CW, MAXDISP = 4, 540, 960, 3, 384, 576, 192.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "transform_probe.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # the copy ceiling, in a process of its own, before this one opens the device
    bw = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bw_probe.py")], capture_output=True, text=True,
                        timeout=600)
    if bw.returncode != 0:
        raise SystemExit("tools/bw_probe.py failed:\n" + bw.stdout + bw.stderr)
    copy_line = [ln for ln in bw.stdout.splitlines() if ln.startswith("copy")][0]
    copy_tbs = float(copy_line.split()[1])

    import torch
    from leastereo_amd import _lib, data
    from tests import transform_judge as J
    if not torch.cuda.is_available():
        raise SystemExit("transform_probe needs the GPU: a timing taken elsewhere says nothing")
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    say(f"{torch.cuda.get_device_name(0)}; B = {B}, {H}x{W}x{PS} uint8 -> {CH}x{CW} float32; median of {a.reps} "
        f"windows of {a.iters} calls [min, max]")
    say(f"tools/bw_probe.py on this box: {copy_line.strip()}")

    rng = np.random.default_rng(0)
    lu = rng.integers(0, 256, (B, H, W, PS), dtype=np.uint8)
    ru = rng.integers(0, 256, (B, H, W, PS), dtype=np.uint8)
    dl = rng.uniform(0, 200, (B, H, W)).astype(np.float32)
    h_lu, h_ru, h_dl = (torch.from_numpy(x).pin_memory() for x in (lu, ru, dl))
    d_lu, d_ru, d_dl = (x.to("cuda") for x in (h_lu, h_ru, h_dl))
    out_l = torch.empty(B, 3, CH, CW, device="cuda")
    out_r = torch.empty_like(out_l)
    out_t = torch.empty(B, 1, CH, CW, device="cuda")
    nv = torch.empty(B, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.lea_train_transform_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    d_params = torch.zeros(B, 5, dtype=torch.int32, device="cuda")

    def launches(ch=CH, cw=CW, l=d_lu, r=d_ru, d=d_dl):
        _lib.check(lib.lea_train_transform_u8(l.data_ptr(), r.data_ptr(), B, H, W, PS, d.data_ptr(), None,
                                              d_params.data_ptr(), out_l.data_ptr(), out_r.data_ptr(),
                                              out_t.data_ptr(), ch, cw, MAXDISP, nv.data_ptr(), ws.data_ptr(),
                                              stream), "lea_train_transform_u8")

    def windows(fn, iters):
        for _ in range(3):
            fn()
        t = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / iters * 1e3)
        return sorted(t)[len(t) // 2], min(t), max(t)

    stats_bytes = 2 * B * H * W * PS
    crop_bytes = 2 * B * CH * CW * PS + B * CH * CW * 4 + 2 * B * 3 * CH * CW * 4 + B * CH * CW * 4
    in_bytes = 2 * B * H * W * PS + B * H * W * 4 + B * 5 * 4
    out_bytes = 2 * B * 3 * CH * CW * 4 + B * CH * CW * 4
    say(f"algorithmic bytes of (a): statistics pass {stats_bytes / 1e6:.2f} MB read, crop pass "
        f"{crop_bytes / 1e6:.2f} MB read + written; (b) copies {in_bytes / 1e6:.2f} MB in, (c) copies "
        f"{out_bytes / 1e6:.2f} MB in")
    for shift in (0, 3):
        tf = data.DeviceTrainTransform(CH, CW, MAXDISP, shift=shift, rng=random.Random(shift))
        h_params = tf.sample(B, H, W)
        d_params.copy_(h_params)
        say(f"shift {shift}: params {h_params.tolist()}")
        # what the launches give is what the host path gives (target and count bitwise)
        launches()
        planes = J.standardize(lu[0], ru[0], dl[0])
        want = J.apply_params(planes, h_params[0].tolist(), CH, CW, has_right_disp=False)
        same_t = bool(np.array_equal(out_t[0].cpu().numpy().view(np.int32), want[2].view(np.int32)))
        same_n = int(nv[0]) == J.n_valid(want[2], MAXDISP)
        ulp = int(np.abs(out_l[0].cpu().numpy().view(np.int32).astype(np.int64) -
                         want[0].view(np.int32).astype(np.int64)).max())
        say(f"  sample 0 vs the host path: target bitwise {same_t}, n_valid equal {same_n}, left image max {ulp} ulp")

        med, lo, hi = windows(launches, a.iters)
        med4, lo4, hi4 = windows(lambda: launches(4, 4), a.iters)
        say(f"  (a) the launches, inputs on the device      {med:9.1f} us [{lo:.1f}, {hi:.1f}]  "
            f"{(stats_bytes + crop_bytes) / med / 1e6:.3f} TB/s of algorithmic bytes "
            f"({(stats_bytes + crop_bytes) / med / 1e6 / copy_tbs:.2f} of the copy figure)")
        say(f"      the entry at a 4x4 crop (clear + statistics){med4:7.1f} us [{lo4:.1f}, {hi4:.1f}]  "
            f"{stats_bytes / med4 / 1e6:.3f} TB/s of the statistics pass's bytes")

        def leg_b():
            l, r, d = (x.to("cuda", non_blocking=True) for x in (h_lu, h_ru, h_dl))
            d_params.copy_(h_params, non_blocking=True)
            launches(l=l, r=r, d=d)

        medb, lob, hib = windows(leg_b, max(1, a.iters // 4))
        say(f"  (b) H2D of uint8 + disparity + params, then (a) {medb:9.1f} us [{lob:.1f}, {hib:.1f}]  "
            f"copy alone {in_bytes / (medb - med) / 1e3:.1f} GB/s")

        host, host_tf = [], []
        pin = [torch.empty(s, dtype=torch.float32).pin_memory() for s in ((B, 3, CH, CW), (B, 3, CH, CW), (B, 1, CH, CW))]
        for _ in range(a.host_reps):
            r = random.Random(shift)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(B):
                t = J.standardize(lu[b], ru[b], dl[b])
                o = J.train_transform(t, CH, CW, shift=shift, rng=r)
                for k in range(3):
                    pin[k][b].copy_(torch.from_numpy(np.ascontiguousarray(o[k])))
            t1 = time.perf_counter()
            dev = [p.to("cuda", non_blocking=True) for p in pin]
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e6)
            host_tf.append((t1 - t0) * 1e6)
        del dev
        mh, mt = sorted(host)[len(host) // 2], sorted(host_tf)[len(host_tf) // 2]
        say(f"  (c) host transform on one core, then H2D of the float32 crops {mh:9.0f} us [{min(host):.0f}, "
            f"{max(host):.0f}]  (transform {mt:.0f} us = {mt / B / 1e3:.1f} ms per sample, copy {mh - mt:.0f} us)")
        say(f"      (c) / (b) = {mh / medb:.1f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
