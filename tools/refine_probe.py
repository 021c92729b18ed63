#!/usr/bin/env python3
"""The disparity refinement (lea_disparity_refine_f32, T = 3) at the bench shapes, in one process:

  * the call through the C ABI on one stream, at T = 1, 2, 3 (the differences are one
    iteration: a horizontal and a vertical pass), and the per-kernel device times of one call
    from torch's profiler (the two directions apart);
  * the plain forward of the same run at the same size (C2, C5), the yardstick;
  * a torch-op restatement: Thomas sweeps vectorised across the lines, one op sequence per
    column or row (what a torch user writes; torch has no tridiagonal solver);
  * the float32 judge of tests/refine_judge.py on the host.

Warmed up, then ``--rounds`` alternating windows of ``--iters`` calls each, HIP events; medians
of the windows with their range.  The torch-op loop and the host judge run once per round.
Writes the lines to ``--out`` as well.

  python tools/refine_probe.py [--iters 20] [--rounds 7] [--out profiles/refine_probe.txt]
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
from tests import refine_judge as rj  # noqa: E402

# (name, B, C, H, W, maxdisp of the forward beside it or None)
SHAPES = [("C2", 1, 3, 576, 960, 192), ("C5", 1, 3, 1008, 1512, 264), ("scene", 1, 3, 2048, 2048, None)]
LAM, SIGMA, T = 8000.0, 0.05, 3


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def torch_thomas(w, num, den, lam):
    """One pass along the last axis with torch ops: w [..., n] (0 at the end), in place."""
    n = num.shape[-1]
    cp = torch.empty_like(num)
    a = torch.zeros_like(num[..., 0])
    cprev, nprev, dprev = a, a, a
    for i in range(n):
        c = -lam * w[..., i]
        inv = 1.0 / (1.0 - a - c - a * cprev)
        cprev = c * inv
        nprev = (num[..., i] - a * nprev) * inv
        dprev = (den[..., i] - a * dprev) * inv
        cp[..., i], num[..., i], den[..., i] = cprev, nprev, dprev
        a = c
    for i in range(n - 2, -1, -1):
        num[..., i] -= cp[..., i] * num[..., i + 1]
        den[..., i] -= cp[..., i] * den[..., i + 1]


def torch_refine(guide, disp, conf, lam, sigma, iterations):
    mh = (guide[..., 1:] - guide[..., :-1]).abs().amax(1)
    mv = (guide[..., 1:, :] - guide[..., :-1, :]).abs().amax(1)
    wh = torch.nn.functional.pad(torch.exp(-mh / sigma), (0, 1))
    wv = torch.nn.functional.pad(torch.exp(-mv / sigma), (0, 0, 0, 1)).transpose(1, 2).contiguous()
    num, den = (conf * disp).contiguous(), conf.clone()
    for lt in rj.schedule(lam, iterations):
        torch_thomas(wh, num, den, lt)
        nt, dt = num.transpose(1, 2).contiguous(), den.transpose(1, 2).contiguous()
        torch_thomas(wv, nt, dt, lt)
        num, den = nt.transpose(1, 2).contiguous(), dt.transpose(1, 2).contiguous()
    return num / den


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
            if "fgs_" in ev.key:
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = ev.cuda_time_total
                out[ev.key.split("(")[0].split("::")[-1]] = (total / ev.count, ev.count // 5)
        try:
            # the sweep kernel's launches in issue order: per call horizontal, vertical, ..., the last vertical
            sweeps = sorted((ev for ev in prof.events() if "fgs_sweep" in ev.name and
                             (getattr(ev, "device_time", 0) or getattr(ev, "cuda_time", 0)) > 0),
                            key=lambda ev: ev.time_range.start)
            per = 2 * T
            if sweeps and len(sweeps) % per == 0:
                us = [getattr(ev, "device_time", 0) or ev.cuda_time for ev in sweeps]
                hor = [u for i, u in enumerate(us) if i % 2 == 0]
                ver = [u for i, u in enumerate(us) if i % 2 == 1 and i % per != per - 1]
                fin = [u for i, u in enumerate(us) if i % per == per - 1]
                out["sweep, horizontal (on the transposed planes)"] = (sum(hor) / len(hor), len(hor) // 5)
                out["sweep, vertical"] = (sum(ver) / len(ver), len(ver) // 5)
                out["sweep, vertical, last (divides and writes the outputs)"] = (sum(fin) / len(fin), len(fin) // 5)
        except Exception:  # an older profiler without per-launch times: the means above stand
            pass
        return out
    except Exception as e:  # the profiler is an extra: the event timings stand without it
        return {"profiler unavailable": (float("nan"), repr(e)[:80])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no_torch_loop", action="store_true", help="skip the torch-op restatement (seconds per call)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "refine_probe.txt"))
    a = ap.parse_args()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; microseconds, median of {a.rounds} alternating windows of {a.iters} "
        f"calls [min, max]; lambda {LAM:g} sigma {SIGMA:g}")
    for name, b, c, h, w, md in SHAPES:
        guide, disp, conf = rj.make_case((b, c, h, w), seed=1)
        g, d, cf = (torch.from_numpy(v).cuda() for v in (guide, disp, conf))
        ws = torch.empty(lib.lea_disparity_refine_workspace_bytes(b, h, w) // 4, device="cuda")
        out, sup = torch.empty_like(d), torch.empty_like(d)

        def call(t):
            _lib.check(lib.lea_disparity_refine_f32(g.data_ptr(), c * h * w, d.data_ptr(), cf.data_ptr(), None, b, c,
                                                    h, w, LAM, SIGMA, t, ws.data_ptr(), out.data_ptr(),
                                                    sup.data_ptr(), stream), "refine")

        fns = [lambda: call(1), lambda: call(2), lambda: call(3)]
        labels = ["T=1", "T=2", "T=3"]
        if md is not None:
            model = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=md)), "cuda").cuda().eval()
            left, right = torch.randn(b, 3, h, w, device="cuda"), torch.randn(b, 3, h, w, device="cuda")

            def forward():
                with torch.no_grad():
                    model(left, right)
            fns.append(forward)
            labels.append("forward")
        for fn in fns:
            fn()
            _timed(fn, 3)
        t = [[] for _ in fns]
        for _ in range(a.rounds):
            for i, fn in enumerate(fns):
                t[i].append(_timed(fn, a.iters if labels[i] != "forward" else max(2, a.iters // 5)))
        med = [sorted(v)[len(v) // 2] for v in t]
        say(f"{name} B={b} C={c} {h}x{w}:")
        for i, lab in enumerate(labels):
            say(f"  {lab:8s} {med[i]:10.1f} us [{min(t[i]):.1f}, {max(t[i]):.1f}]")
        say(f"  one iteration (T=3 - T=2) {med[2] - med[1]:8.1f} us; (T=2 - T=1) {med[1] - med[0]:8.1f} us")
        if md is not None:
            say(f"  refinement (T=3) / forward = {med[2] / med[3]:.4f}")
            del model
        for k, (us, n) in sorted(kernel_times(lambda: call(3)).items()):
            say(f"  kernel {k}: {us:8.1f} us mean, {n} launches per call")
        call(3)
        got = out.cpu().numpy()
        t0 = time.time()
        w32 = rj.refine32(guide, disp, conf, None, LAM, SIGMA, T)
        host = time.time() - t0
        say(f"  refine32 on the host (numpy) {host * 1e3:8.1f} ms; max |GPU - refine32| "
            f"{float(np.abs(got - w32['refined']).max()):.3e} px")
        if not a.no_torch_loop:
            tt = []
            for _ in range(3):
                tt.append(_timed(lambda: torch_refine(g, d, cf, LAM, SIGMA, T), 1))
            res = torch_refine(g, d, cf, LAM, SIGMA, T)
            say(f"  torch-op Thomas loop {sorted(tt)[1] / 1e3:8.1f} ms [{min(tt) / 1e3:.1f}, {max(tt) / 1e3:.1f}]; "
                f"torch loop / T=3 call {sorted(tt)[1] / med[2]:.0f}x; max |GPU - torch loop| "
                f"{float((res - out).abs().max()):.3e} px")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
