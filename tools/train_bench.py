"""Times one training step of the matching path on the GPU:
cost volume -> newMatching in train mode -> Disp -> smooth_l1 -> backward, on the HIP
ops (leastereo_amd.training), and the same step with every op swapped for torch's
own (F.conv3d / F.batch_norm / F.interpolate on MIOpen: the reference's aten path on
this GPU) -- a measurement tool, not part of the product.  Also times ConvBR3d
forward + backward alone at the hot layer shapes.  One JSON line per measurement.

    python tools/train_bench.py [--height 288 --width 576 --maxdisp 96] [--steps 5]
    python tools/train_bench.py --edge_loss_w 0.2 ...   the reference's combined_loss (train.py:107-113)
    python tools/train_bench.py --whole 1 --photo_loss_w 0.1   adds W x losses.photometric_loss to the whole-model step
                                                        (--whole 2: with and without it in one process)
    python tools/train_bench.py --whole 1 --device_transform 1 [--src_height 540 --src_width 960]
                                                        the loader's transform inside the timed step
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from leastereo_amd import losses, training  # noqa: E402
from leastereo_amd.config import LEAStereoArgs, default_arch_args  # noqa: E402
from leastereo_amd.model import LEAStereo  # noqa: E402


def _torch_convbr(m, x, train):
    y = F.conv3d(x, m.conv.weight, padding=m.conv.weight.shape[-1] // 2)
    if m.use_bn:
        y = F.batch_norm(y, m.bn.running_mean, m.bn.running_var, m.bn.weight, m.bn.bias, train, m.bn.momentum,
                         m.bn.eps)
    return F.relu(y) if m.relu else y


def _torch_interp(x, size, align_corners=True):
    return F.interpolate(x, list(size), mode="trilinear", align_corners=align_corners)


def _torch_cost(fl, fr, maxdisp):
    d3, c = int(maxdisp / 3), fl.shape[1]
    cost = fl.new_zeros(fl.shape[0], 2 * c, d3, fl.shape[2], fl.shape[3])
    for i in range(d3):
        cost[:, :c, i, :, i:] = fl[:, :, :, i:]
        cost[:, c:, i, :, i:] = fr[:, :, :, :-i] if i > 0 else fr
    return cost


def _torch_disp(cost, maxdisp):
    u = F.interpolate(cost, [maxdisp, cost.shape[3] * 3, cost.shape[4] * 3], mode="trilinear", align_corners=False)
    p = F.softmax(-torch.squeeze(u, 1), dim=1)
    return torch.sum(p * torch.arange(maxdisp, device=cost.device, dtype=p.dtype).view(1, maxdisp, 1, 1), 1)


def _torch_combined_loss(disp, target, tsmooth, maxdisp, w):
    """train.py:107-118 and edge_detection.py:68-74 from torch ops; ``tsmooth`` is the
    twice-median target, formed once outside the timed region (the reference forms it on
    the host with cv2 every step; cv2 is not available here, so that round trip is not part
    of this leg -- tools/loss_probe.py times a scipy stand-in for it)."""
    mask = (target < maxdisp) & (target > 0.001)
    direct = F.smooth_l1_loss(disp[mask], target[mask], reduction="mean")
    kx = disp.new_tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]).view(1, 1, 3, 3)
    ky = disp.new_tensor([[1, 2, 1], [0, 0, 0], [-1, -2, -1]]).view(1, 1, 3, 3)
    ox, oy = F.conv2d(disp.unsqueeze(1), kx), F.conv2d(disp.unsqueeze(1), ky)
    tx, ty = F.conv2d(tsmooth.unsqueeze(1), kx), F.conv2d(tsmooth.unsqueeze(1), ky)
    edge = torch.mean(torch.abs(ox) * torch.exp(-torch.abs(tx)) + torch.abs(oy) * torch.exp(-torch.abs(ty)))
    return direct + edge * w


def _loss(disp, target, tsmooth, maxdisp, edge_loss_w, impl):
    if not edge_loss_w:
        return None
    if impl == "torch":
        return _torch_combined_loss(disp, target, tsmooth, maxdisp, edge_loss_w)
    return losses.combined_loss(disp, target, maxdisp, edge_loss_w)


def step_fn(model, fl, fr, target, impl, edge_loss_w=0.0, tsmooth=None):
    if impl == "torch":
        saved = training._convbr, training.interpolate3d
        training._convbr, training.interpolate3d = _torch_convbr, _torch_interp
        try:
            disp = _torch_disp(training.matching_forward(model.matching, _torch_cost(fl, fr, model.maxdisp)),
                               model.maxdisp)
        finally:
            training._convbr, training.interpolate3d = saved
    else:
        disp = training.cost_to_disparity_train(model, fl, fr)
    loss = _loss(disp, target, tsmooth, model.maxdisp, edge_loss_w, impl)
    if loss is None:
        loss = F.smooth_l1_loss(disp, target)
    loss.backward()
    return loss


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--width", type=int, default=576)
    ap.add_argument("--maxdisp", type=int, default=96)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--impl", default="hip,torch")
    ap.add_argument("--whole", type=int, default=0, help="1: time only the whole-model train step; 2: that step with the plain loss and with "
                         "--edge_loss_w (0.2 if not given) in alternating windows of one process")
    ap.add_argument("--edge_loss_w", type=float, default=0.0,
                    help="> 0: the step's loss is the reference's combined_loss with this weight "
                         "(leastereo_amd.losses on the hip impl, torch ops on the torch impl); 0: off")
    ap.add_argument("--photo_loss_w", type=float, default=0.0,
                    help="> 0 (with --whole 1 or 2): adds this weight times losses.photometric_loss(left, right, disp) "
                         "to the step's loss, next to --edge_loss_w; 0: off")
    ap.add_argument("--device_transform", type=int, default=0,
                    help="1 (with --whole 1): the step starts from decoded uint8 pairs of --src_height x "
                         "--src_width and their disparity, standardised, random-cropped to --height x --width "
                         "and cut to the target on the device (leastereo_amd.data.DeviceTrainTransform)")
    ap.add_argument("--warp_aug", type=float, default=0.0, metavar="P",
                    help="> 0 (with --whole 1): after the plain step, time the step with "
                         "leastereo_amd.synthesis.DisparityScaleAugment(prob=P) in front of it -- the right view "
                         "re-synthesised from the left image and the target (the data here is synthetic, so "
                         "the from-left path) -- and print it on a second line beside the plain one; 0: off")
    ap.add_argument("--src_height", type=int, default=540)
    ap.add_argument("--src_width", type=int, default=960)
    ap.add_argument("--torch-modes", default="default,benchmark",
                    help="MIOpen modes for the torch leg: default (immediate mode) and/or benchmark "
                         "(torch.backends.cudnn.benchmark=True: MIOpen's find per shape, more warm-up)")
    args = ap.parse_args()
    torch.backends.cudnn.allow_tf32 = False
    dev = "cuda"
    if args.whole:
        return whole_model(args, dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    # ConvBR3d forward + backward at the hot shapes (C2's L0 8->8 cell, L1 16->16, conv1)
    for name, (cin, cout, d, h, w) in {"L0_8to8": (8, 8, 64, 192, 320), "L1_16to16": (16, 16, 32, 96, 160),
                                       "conv1_128to64": (128, 64, 32, 96, 160)}.items():
        m = training.ConvBR3d(cin, cout, 3, 1, 1).to(dev).train()
        x = torch.randn(1, cin, d, h, w, device=dev, generator=gen).requires_grad_(True)
        dy = torch.randn(1, cout, d, h, w, device=dev, generator=gen)
        ms = timed(lambda: m(x).backward(dy), args.steps, args.warmup)
        fl = 2.0 * cin * cout * 27 * d * h * w  # one direct conv: 2 FLOPs per MAC
        # forward + data gradient + weight gradient = three convs' work
        print(json.dumps({"what": "convbr3d_fwd_bwd", "layer": name, "ms": round(ms, 3),
                          "direct_tflops": round(3 * fl / ms / 1e9, 1)}), flush=True)
    model = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=args.maxdisp)), dev).to(dev).train()
    h3, w3 = (args.height - 1) // 3 + 1, (args.width - 1) // 3 + 1
    fl = torch.randn(1, 32, h3, w3, device=dev, generator=gen).requires_grad_(True)
    fr = torch.randn(1, 32, h3, w3, device=dev, generator=gen).requires_grad_(True)
    target = torch.rand(1, 3 * h3, 3 * w3, device=dev, generator=gen) * args.maxdisp
    tsmooth = losses.smooth_target(target) if args.edge_loss_w else None
    for impl in args.impl.split(","):
        for mode in (args.torch_modes.split(",") if impl == "torch" else ["-"]):
            torch.backends.cudnn.benchmark = mode == "benchmark"
            warm = args.warmup + (3 if mode == "benchmark" else 0)
            t0 = time.perf_counter()
            ms = timed(lambda: step_fn(model, fl, fr, target, impl, args.edge_loss_w, tsmooth), args.steps, warm)
            print(json.dumps({"what": "matching_train_step", "impl": impl, "miopen_mode": mode,
                              "edge_loss_w": args.edge_loss_w,
                              "height": args.height, "width": args.width, "maxdisp": args.maxdisp,
                              "ms": round(ms, 2), "warmup_steps": warm,
                              "wall_s": round(time.perf_counter() - t0, 1),
                              "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}), flush=True)


def whole_model(args, dev):
    """train.py:150-158 on the drop-in: model.train(), model(left, right) with inputs that
    require grad, smooth_l1, backward, SGD step -- the whole model (feature net twice,
    cost volume, matching net, Disp) on the HIP library."""
    model = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=args.maxdisp)), dev).to(dev).train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-4, momentum=0.9)
    gen = torch.Generator(device=dev).manual_seed(1)
    left = torch.randn(1, 3, args.height, args.width, device=dev, generator=gen).requires_grad_(True)
    right = torch.randn(1, 3, args.height, args.width, device=dev, generator=gen).requires_grad_(True)
    target = torch.rand(1, args.height, args.width, device=dev, generator=gen) * (args.maxdisp - 1)

    tf = None
    if args.device_transform:
        # the loader's per-sample transform inside the timed step: decoded uint8 pairs and
        # disparities (synthetic, already on the device) through leastereo_amd.data
        from leastereo_amd.data import DeviceTrainTransform
        src = (1, args.src_height, args.src_width)
        left_u8 = torch.randint(0, 256, src + (3,), device=dev, dtype=torch.uint8, generator=gen)
        right_u8 = torch.randint(0, 256, src + (3,), device=dev, dtype=torch.uint8, generator=gen)
        disp_u8 = torch.rand(src, device=dev, generator=gen) * (args.maxdisp - 1)
        tf = DeviceTrainTransform(args.height, args.width, args.maxdisp, device=dev)

    aug = None
    if args.warp_aug:
        from leastereo_amd.synthesis import DisparityScaleAugment
        aug = DisparityScaleAugment(prob=args.warp_aug, device=dev, maxdisp=args.maxdisp)

    def step(edge_loss_w=args.edge_loss_w, photo_loss_w=args.photo_loss_w, warp=False):
        nonlocal left, right, target
        opt.zero_grad()
        if tf is not None:
            batch = tf(left_u8, right_u8, disp_u8)
            left, right = batch.left.requires_grad_(True), batch.right.requires_grad_(True)
            target = batch.target.squeeze(1)
        if warp:  # a fresh scale every step; the plain step's tensors stay as they are
            pair = aug(left.detach(), right.detach(), target)
            return finish(left, pair.right.requires_grad_(True), pair.disp_left, edge_loss_w, photo_loss_w)
        return finish(left, right, target, edge_loss_w, photo_loss_w)

    def finish(left, right, target, edge_loss_w, photo_loss_w):
        disp = model(left, right)
        if edge_loss_w:
            loss = losses.combined_loss(disp, target, args.maxdisp, edge_loss_w)
        else:
            mask = (target < args.maxdisp) & (target > 0.001)
            loss = F.smooth_l1_loss(disp[mask], target[mask], reduction="mean")
        if photo_loss_w:
            loss = loss + photo_loss_w * losses.photometric_loss(left, right, disp)
        loss.backward()
        opt.step()
    torch.cuda.reset_peak_memory_stats()
    if args.whole == 2:
        # processes differ by more than the loss costs: both steps in this one, in alternating
        # windows of --steps steps, the order reversed every other round; medians of the windows
        # (with --photo_loss_w: the step with and without the photometric term instead)
        photo = bool(args.photo_loss_w)
        ws = (0.0, args.photo_loss_w) if photo else (0.0, args.edge_loss_w or 0.2)
        run = (lambda w: step(args.edge_loss_w, w)) if photo else (lambda w: step(w, 0.0))
        t = {w: [] for w in ws}
        for w in ws:
            timed(lambda: run(w), 1, args.warmup)
        for r in range(7):
            for w in (ws if r % 2 == 0 else ws[::-1]):
                t[w].append(timed(lambda: run(w), args.steps, 0))
        for w in ws:
            v = sorted(t[w])
            print(json.dumps({"what": "whole_model_train_step_ab", "impl": "hip", "height": args.height,
                              "width": args.width, "maxdisp": args.maxdisp,
                              "edge_loss_w": args.edge_loss_w if photo else w, **({"photo_loss_w": w} if photo else {}),
                              "ms_median": round(v[len(v) // 2], 2), "ms_min": round(v[0], 2),
                              "ms_max": round(v[-1], 2), "windows": len(v), "steps_per_window": args.steps}),
                  flush=True)
        return
    ms = timed(step, args.steps, args.warmup)
    line = {"what": "whole_model_train_step", "impl": "hip", "height": args.height, "width": args.width,
            "maxdisp": args.maxdisp, "edge_loss_w": args.edge_loss_w, "ms": round(ms, 2),
            "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
    if args.photo_loss_w:  # the default line keeps its keys
        line["photo_loss_w"] = args.photo_loss_w
    if tf is not None:
        line.update({"device_transform": 1, "src_height": args.src_height, "src_width": args.src_width})
    print(json.dumps(line), flush=True)
    if aug is not None:  # the same step behind the augmentation, in the same process
        ms_aug = timed(lambda: step(warp=True), args.steps, args.warmup)
        print(json.dumps(dict(line, what="whole_model_train_step_warp_aug", warp_aug=args.warp_aug, ms_plain=line["ms"],
                              ms=round(ms_aug, 2))), flush=True)


if __name__ == "__main__":
    main()
