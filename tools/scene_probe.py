#!/usr/bin/env python3
"""Whole-scene inference at 2048 x 2048 x 3 (tile 576 x 960, maxdisp 192), in one process:

  (a) the gather launch (lea_standardize_tiles_u8) and the blend launch (lea_tile_blend_f32,
      left and right view), in us and as the HBM rate of the bytes they must move;
  (b) the same gather and blend composed from torch ops (float statistics, slicing and
      ``stack``; weight tensors, ``index_add_`` and a divide);
  (c) the host path of the blend: a D2H copy of the tiles, the numpy judge
      (tests/scene_judge.py) and an H2D copy of the result;
  (d) the whole ``SceneRunner`` call against N x the replay of the same graph alone.

Warmed up, HIP events, the median of ``--iters`` single calls with their range.  Run once
per setting; appends to ``--out``.

  python tools/scene_probe.py [--precision f32] [--tile_batch 1] [--iters 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from leastereo_amd import kernels, scene  # noqa: E402
from leastereo_amd.config import LEAStereoArgs, default_arch_args  # noqa: E402
from leastereo_amd.model import LEAStereo  # noqa: E402
from tests import scene_judge  # noqa: E402

H = W = 2048
TH, TW, MD = 576, 960, 192


def _events(fn, iters, warmup=3):
    """Median, min and max in us of single calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def _fmt(name, t, nbytes=None):
    s = f"{name:<44s} {t[0]:10.1f} us  [{t[1]:.1f} .. {t[2]:.1f}]"
    if nbytes:
        s += f"  {nbytes / 1e6:8.1f} MB -> {nbytes / t[0] / 1e6:6.2f} TB/s"
    return s


def torch_gather(left, right, origins):
    """(b): float statistics, a standardised scene, N slices stacked (scenes that need no pad)."""
    out = []
    for img in (left, right):
        x = img[..., :3].permute(2, 0, 1).double()
        x = ((x - x.mean((1, 2), keepdim=True)) / x.std((1, 2), unbiased=False, keepdim=True)).float()
        out.append(torch.stack([x[:, oy:oy + TH, ox:ox + TW] for oy, ox in origins]))
    return out


def torch_blend(tiles, weights, flat_index, den):
    """(b): index_add_ of the weighted tiles into the scene, then the divide.  The weight
    tensors, the scatter indices and the denominator are made once, outside the timing."""
    num = torch.zeros(H * W, device=tiles.device)
    num.index_add_(0, flat_index, (tiles * weights).flatten())
    return (num / den).view(H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--tile_batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scene_probe.txt"))
    a = ap.parse_args()
    dev = "cuda"
    rng = np.random.default_rng(0)
    left = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    right = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    torch.manual_seed(0)
    model = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), dev, precision=a.precision).to(dev).eval()
    runner = scene.SceneRunner(model, TH, TW, tile_batch=a.tile_batch)
    plan = runner.plan(H, W)
    n = len(plan)
    lines = [f"# scene {H}x{W}x3, tile {TH}x{TW}, maxdisp {MD}, {a.precision}, tile_batch {a.tile_batch}: "
             f"{plan.ny} x {plan.nx} = {n} tiles, context {plan.context}, ramp {plan.ramp}; "
             f"{torch.cuda.get_device_name(0)}; median of {a.iters} [min .. max]"]
    origins_dev = torch.from_numpy(plan.origins).to(dev)
    origins = plan.origins.tolist()

    # (a) the two kernels
    gather_bytes = 2 * (H * W * 3 * 2 + n * 3 * TH * TW * 4)  # the scene twice (statistics, tiles), the tiles out
    t = _events(lambda: kernels.standardize_tiles_u8(left, right, origins_dev, TH, TW), a.iters)
    lines.append(_fmt("(a) gather: lea_standardize_tiles_u8", t, gather_bytes))
    tiles = torch.randn((n, TH, TW), device=dev)
    for view in ("left", "right"):
        cover = plan.cover_count(view)
        blend_bytes = int(cover.sum()) * 4 + H * W * 4  # each covering tile value once, the map out
        t = _events(lambda: kernels.blend_tiles(tiles, plan, view), a.iters)
        lines.append(_fmt(f"(a) blend ({view}): lea_tile_blend_f32", t, blend_bytes))
    t = _events(lambda: kernels.blend_tiles(tiles, plan, "left", count=torch.empty(1, dtype=torch.int32, device=dev)),
                a.iters)
    lines.append(_fmt("(a) blend (left) with the hole count", t))

    # (b) torch ops
    t = _events(lambda: torch_gather(left, right, origins), a.iters)
    lines.append(_fmt("(b) gather from torch ops", t))
    weights = torch.stack([torch.from_numpy(plan.weights(k, "left")).float() for k in range(n)]).to(dev)
    yy = torch.arange(TH, device=dev).view(1, TH, 1) + origins_dev[:, 0].view(n, 1, 1)
    xx = torch.arange(TW, device=dev).view(1, 1, TW) + origins_dev[:, 1].view(n, 1, 1)
    flat_index = (yy * W + xx).flatten().long()
    den = torch.zeros(H * W, device=dev).index_add_(0, flat_index, weights.flatten())
    t = _events(lambda: torch_blend(tiles, weights, flat_index, den), a.iters)
    lines.append(_fmt("(b) blend from torch ops (index_add_, divide)", t))
    got = kernels.blend_tiles(tiles, plan, "left")
    diff = float((torch_blend(tiles, weights, flat_index, den) - got).abs().max())
    lines.append(f"    max |torch blend - kernel blend| = {diff:.3e}")

    # (c) the host path of one blend
    def host_blend():
        host = tiles.cpu().numpy()
        out, _ = scene_judge.blend(host, plan.ys, plan.xs, H, W, MD, plan.context, plan.ramp, "left")
        return torch.from_numpy(out).to(dev)
    t0 = time.perf_counter()
    want = host_blend()
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t0
    lines.append(f"{'(c) blend on the host (D2H, numpy, H2D), one call':<44s} {host_s * 1e6:10.1f} us; equal to the kernel's "
                 f"bit for bit: {bool(torch.equal(want, got))}")

    # (d) the whole call against its forwards alone
    t_run = _events(lambda: runner(left, right), a.iters, warmup=2)
    graph = runner._graphs["plain"]
    t_fwd = _events(lambda: graph.graph.replay(), a.iters)
    nb = len(runner.batches(plan))
    lines.append(_fmt(f"(d) runner(left, right): {nb} replays of batch {a.tile_batch}", t_run))
    lines.append(_fmt("(d) one replay of that graph alone", t_fwd))
    lines.append(f"    whole call / ({nb} x replay) = {t_run[0] / (nb * t_fwd[0]):.3f}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n\n")


if __name__ == "__main__":
    main()
