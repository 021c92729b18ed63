#!/usr/bin/env python3
"""The speckle filter (lea_disparity_speckle_f32, all four outputs) at the bench shapes, in
one process:

  * the call through the C ABI on one stream on four fields: the model-like recipe of the
    tests (piecewise-smooth blocks plus salt, walls and NaNs), a constant image (one component),
    a one-pixel checkerboard at max_diff 0 (every pixel its own component) and a serpentine
    (one component that crosses every tile border); the per-kernel device times of one call
    from torch's profiler;
  * beside them the same run's plain forward (C2, C5) and the same run's ``fgs_refine`` call
    (T = 3) at the same size, the yardsticks;
  * the host path that the call replaces: device-to-host copy, connected components on the
    host (scipy.sparse.csgraph on the edge list where scipy is importable, else the numpy
    judge), host-to-device copy of the state; its labels and sizes are compared with the
    call's, every pixel.

Warmed up, then ``--rounds`` alternating windows of ``--iters`` calls each, HIP events; medians
of the windows with their range.  The host path runs once per field.  Writes the lines to
``--out`` as well.

  python tools/speckle_probe.py [--iters 20] [--rounds 7] [--out profiles/speckle_probe.txt]
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
from tests import speckle_judge as sj  # noqa: E402

# (name, B, H, W, maxdisp of the forward beside it or None)
SHAPES = [("C2", 1, 576, 960, 192), ("C5", 1, 1008, 1512, 264), ("scene", 1, 2048, 2048, None)]
MAX_SIZE = 200


def fields(b, h, w):
    """(name, disp [B, H, W], exclude or None, max_diff)"""
    d, e = sj.random_field((b, h, w), seed=1)
    yield "model-like", d, e, 1.0
    yield "constant", np.full((b, h, w), 7.25, np.float32), None, 1.0
    yield "checkerboard", np.broadcast_to(sj.checkerboard(h, w), (b, h, w)).copy(), None, 0.0
    yield "serpentine", np.broadcast_to(sj.serpentine(h, w), (b, h, w)).copy(), None, 1.0


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
            if "speckle_" in ev.key:
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = ev.cuda_time_total
                out[ev.key.split("(")[0].split("::")[-1]] = (total / ev.count, ev.count // 5)
        return out
    except Exception as e:  # the profiler is an extra: the event timings stand without it
        return {"profiler unavailable": (float("nan"), repr(e)[:80])}


def host_components(d, e, max_diff):
    try:
        import scipy  # noqa: F401
        return "scipy csgraph", sj.labels_by_graph(d, e, max_diff)
    except ImportError:
        return "numpy propagation", sj.labels_by_propagation(d, e, max_diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "speckle_probe.txt"))
    a = ap.parse_args()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; microseconds, median of {a.rounds} alternating windows of {a.iters} "
        f"calls [min, max]; max_size {MAX_SIZE}, max_diff 1 (checkerboard: 0); labels, size, state and filtered "
        f"written")
    for name, b, h, w, md in SHAPES:
        n = b * h * w
        ws = torch.empty(lib.lea_disparity_speckle_workspace_bytes(b, h, w) // 4, device="cuda", dtype=torch.int32)
        labels = torch.empty((b, h, w), device="cuda", dtype=torch.int32)
        size = torch.empty_like(labels)
        state = torch.empty((b, h, w), device="cuda", dtype=torch.uint8)
        filt = torch.empty((b, h, w), device="cuda", dtype=torch.float32)
        cases = [(fname, torch.from_numpy(d).cuda(), None if e is None else torch.from_numpy(e).cuda(), mdiff, d, e)
                 for fname, d, e, mdiff in fields(b, h, w)]

        def call(case):
            _, dd, ee, mdiff, _, _ = case
            _lib.check(lib.lea_disparity_speckle_f32(dd.data_ptr(), None if ee is None else ee.data_ptr(), b, h, w,
                                                     mdiff, MAX_SIZE, 0.0, ws.data_ptr(), labels.data_ptr(),
                                                     size.data_ptr(), state.data_ptr(), filt.data_ptr(), stream),
                       "speckle")

        fns = [(lambda c=c: call(c)) for c in cases]
        names = [c[0] for c in cases]
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
        for i, lab in enumerate(names):
            say(f"  {lab:13s} {med[i]:10.1f} us [{min(t[i]):.1f}, {max(t[i]):.1f}]")
        ref = med[names.index("fgs_refine")]
        say("  call / fgs_refine: " + ", ".join(f"{names[i]} {med[i] / ref:.3f}" for i in range(len(cases))))
        say("  call / model-like: " + ", ".join(f"{names[i]} {med[i] / med[0]:.2f}" for i in range(1, len(cases))))
        if md is not None:
            say(f"  model-like call / forward = {med[0] / med[names.index('forward')]:.5f}")
            del model
        for case in cases:
            for k, (us, cnt) in sorted(kernel_times(lambda: call(case)).items()):
                say(f"  {case[0]:13s} kernel {k}: {us:8.1f} us mean, {cnt} launch per call")
        for case in cases:
            fname, dd, ee, mdiff, d, e = case
            call(case)
            torch.cuda.synchronize()
            t0 = time.time()
            dh = dd.cpu().numpy()
            eh = None if ee is None else ee.cpu().numpy()
            t1 = time.time()
            how, (hl, hs) = host_components(dh, eh, mdiff)
            hstate = np.where((hs > 0) & (hs <= MAX_SIZE), 3, 0).astype(np.uint8)
            t2 = time.time()
            torch.from_numpy(hstate).cuda()
            torch.cuda.synchronize()
            t3 = time.time()
            same = np.array_equal(labels.cpu().numpy(), hl) and np.array_equal(size.cpu().numpy(), hs)
            comps = int((hl == np.arange(h * w).reshape(1, h, w)).sum())
            say(f"  {fname:13s} host path ({how}): copy out {1e3 * (t1 - t0):.1f} ms, components "
                f"{1e3 * (t2 - t1):.1f} ms, copy in {1e3 * (t3 - t2):.1f} ms; {comps} components, largest "
                f"{int(hs.max())} px; the call's labels and sizes equal the host's: {same}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
