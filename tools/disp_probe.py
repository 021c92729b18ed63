#!/usr/bin/env python3
"""The disparity regression at the bench shapes, every form (lea_disparity_set_register_form
1 / 2 / 3 / 4 / 0, in that order), f32 and fast exp: HIP-event microseconds and the largest
difference from form 1.

  python tools/disp_probe.py [--iters 20]
  python tools/disp_probe.py --stats [--iters 20] [--rounds 9]   the confidence head beside the plain one
  python tools/disp_probe.py --lr [--iters 20] [--rounds 9]      the right head and the left-right check beside it
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leastereo_amd import _lib, kernels  # noqa: E402

SHAPES = [("C2", 1, 64, 192, 320, 192), ("C4", 8, 64, 192, 320, 192), ("C3", 8, 64, 128, 416, 192),
          ("C5", 1, 88, 336, 504, 264)]


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def stats_main(a, lib):
    """lea_disparity_regression_stats (all four outputs, radius 4) next to the plain entry in
    its default form: the same cost and disparity buffers, launched through the C ABI on one
    stream, warmed up, then ``--rounds`` alternating windows of ``--iters`` launches each;
    medians of the windows, and whether the two disparities are the same bits."""
    g = torch.Generator(device="cuda").manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream
    for name, b, d3, h3, w3, md in SHAPES:
        if name not in ("C2", "C4", "C5"):
            continue
        x = torch.randn(b, 1, d3, h3, w3, device="cuda", generator=g) * 3
        disp, ent, peak, loc = (torch.empty(b, 3 * h3, 3 * w3, device="cuda") for _ in range(4))
        for fast in (False, True):
            dt = _lib.LEA_BF16 if fast else _lib.LEA_F32

            def plain():
                _lib.check(lib.lea_disparity_regression(x.data_ptr(), disp.data_ptr(), b, d3, h3, w3, md, dt,
                                                        stream), "plain")

            def stats():
                _lib.check(lib.lea_disparity_regression_stats(
                    x.data_ptr(), disp.data_ptr(), ent.data_ptr(), peak.data_ptr(), loc.data_ptr(), b, d3, h3,
                    w3, md, 4, dt, stream), "stats")

            plain()
            want = disp.clone()
            stats()
            same = bool(torch.equal(want, disp))
            for fn in (plain, stats):
                _timed(fn, a.iters)
            tp, ts = [], []
            for _ in range(a.rounds):
                tp.append(_timed(plain, a.iters))
                ts.append(_timed(stats, a.iters))
            mp, ms = sorted(tp)[len(tp) // 2], sorted(ts)[len(ts) // 2]
            print(f"{name} B={b} D3={d3} {3 * h3}x{3 * w3} fast={int(fast)}  plain {mp:7.1f} us "
                  f"[{min(tp):.1f}, {max(tp):.1f}]  stats {ms:7.1f} us [{min(ts):.1f}, {max(ts):.1f}]  "
                  f"stats / plain {ms / mp:.2f}  disp same bits: {same}", flush=True)


def lr_main(a, lib):
    """lea_disparity_regression_right and lea_disparity_lr_check (both outputs, threshold 1)
    next to the plain entry in its default form, at C2 and C5: one cost, launched through the
    C ABI on one stream, warmed up, then ``--rounds`` alternating windows of ``--iters``
    launches each; medians of the windows.  The check runs on the two heads' outputs."""
    g = torch.Generator(device="cuda").manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream
    for name, b, d3, h3, w3, md in SHAPES:
        if name not in ("C2", "C5"):
            continue
        x = torch.randn(b, 1, d3, h3, w3, device="cuda", generator=g) * 3
        disp, right, filled = (torch.empty(b, 3 * h3, 3 * w3, device="cuda") for _ in range(3))
        state = torch.empty(b, 3 * h3, 3 * w3, device="cuda", dtype=torch.uint8)
        for fast in (False, True):
            dt = _lib.LEA_BF16 if fast else _lib.LEA_F32

            def plain():
                _lib.check(lib.lea_disparity_regression(x.data_ptr(), disp.data_ptr(), b, d3, h3, w3, md, dt,
                                                        stream), "plain")

            def rhead():
                _lib.check(lib.lea_disparity_regression_right(x.data_ptr(), right.data_ptr(), b, d3, h3, w3, md,
                                                              dt, stream), "right")

            def check():
                _lib.check(lib.lea_disparity_lr_check(disp.data_ptr(), right.data_ptr(), state.data_ptr(),
                                                      filled.data_ptr(), b, 3 * h3, 3 * w3, 1.0, stream), "check")

            fns = (plain, rhead, check)
            for fn in fns:
                fn()
                _timed(fn, a.iters)
            t = [[] for _ in fns]
            for _ in range(a.rounds):
                for i, fn in enumerate(fns):
                    t[i].append(_timed(fn, a.iters))
            med = [sorted(v)[len(v) // 2] for v in t]
            flagged = float((state != 0).float().mean())
            print(f"{name} B={b} D3={d3} {3 * h3}x{3 * w3} fast={int(fast)}  plain {med[0]:7.1f} us "
                  f"[{min(t[0]):.1f}, {max(t[0]):.1f}]  right {med[1]:7.1f} us [{min(t[1]):.1f}, {max(t[1]):.1f}]  "
                  f"check {med[2]:7.1f} us [{min(t[2]):.1f}, {max(t[2]):.1f}]  right / plain {med[1] / med[0]:.2f}  "
                  f"flagged {flagged:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--stats", action="store_true",
                    help="time lea_disparity_regression_stats next to the plain entry (C2, C4, C5)")
    ap.add_argument("--lr", action="store_true",
                    help="time lea_disparity_regression_right and lea_disparity_lr_check next to the plain "
                         "entry (C2, C5)")
    ap.add_argument("--rounds", type=int, default=9, help="--stats / --lr: alternating timed windows per entry")
    a = ap.parse_args()
    lib = _lib.load()
    if a.stats:
        return stats_main(a, lib)
    if a.lr:
        return lr_main(a, lib)
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, b, d3, h3, w3, md in SHAPES:
        x = torch.randn(b, 1, d3, h3, w3, device="cuda", generator=g) * 3
        for fast in (False, True):
            out = {}
            for form in (1, 2, 3, 4, 0):
                _lib.check(lib.lea_disparity_set_register_form(form), "form")
                out[form] = kernels.disparity_regression(x, md, fast)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    kernels.disparity_regression(x, md, fast)
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) / a.iters * 1e3
                print(f"{name} fast={int(fast)} form={form} {us:8.1f} us  max|d - form1| "
                      f"{float((out[form] - out.get(1, out[form])).abs().max()):.2e}"
                      + (f"  form 3 == form 2: {bool(torch.equal(out[3], out[2]))}" if form == 3 else ""),
                      flush=True)
    _lib.check(lib.lea_disparity_set_register_form(4), "form")


if __name__ == "__main__":
    main()
