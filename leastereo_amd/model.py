"""Drop-in ``LEAStereo(args, device)`` whose hot path runs on hand-written HIP kernels.

Mirrors retrain/LEAStereo.py:12-52: same constructor arguments, same
state_dict keys (918 tensors; ``load_state_dict(strict=True)`` of a reference
checkpoint works), same ``forward(left, right) -> [B, H, W]`` disparity.

Everything runs on libleastereo_hip.so (``kernels.py``): the 2D feature net
(retrain/new_model_2d.py, ``FeatureExecutor``; north_star allowed it to stay on
PyTorch -- moved to HIP as SURVEY.md §8f rank 2), the cost volume, the matching net
(``MatchingExecutor``) and the disparity regression.  The nn.Modules here are
parameter containers with the reference's names; there is no torch/CPU compute
path: forward on a non-ROCm device raises.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

# the fused feature stem reads left and right directly (two launches, no concatenated
# copy); LEASTEREO_STEM_PAIR=0 stacks the images first (one launch + a torch copy)
STEM_PAIR = os.environ.get("LEASTEREO_STEM_PAIR", "1") != "0"

from . import kernels
from .arch import (PRIMITIVES_2D, PRIMITIVES_3D, cell_specs, check_matching_shape,
                   network_layer_to_space, ops_in_iteration_order, scale_dimension)


# ----------------------------------------------------------------- parameter modules
class ConvBR(nn.Module):
    """Conv (no bias) + BN + ReLU, key-compatible with models/operations_{2d,3d}.py:31."""

    def __init__(self, c_in, c_out, kernel_size, stride=1, padding=0, bn=True, relu=True, dims=3):
        super().__init__()
        conv = nn.Conv3d if dims == 3 else nn.Conv2d
        norm = nn.BatchNorm3d if dims == 3 else nn.BatchNorm2d
        self.relu = relu
        self.use_bn = bn
        self.stride = stride
        self.padding = padding
        self.conv = conv(c_in, c_out, kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = norm(c_out)
        for m in self.modules():  # operations_3d.py:49-55
            if isinstance(m, (nn.Conv2d, nn.Conv3d)):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    @torch.no_grad()
    def folded_bn(self):
        """scale = gamma/sqrt(var+eps), shift = beta - mean*scale, in fp32 as aten's
        batch_norm inference transform folds them."""
        if not self.use_bn:
            return None, None
        bn = self.bn
        invstd = 1.0 / torch.sqrt(bn.running_var.float() + bn.eps)
        scale = invstd * bn.weight.float()
        shift = bn.bias.float() - bn.running_mean.float() * scale
        return scale.contiguous(), shift.contiguous()


class Cell(nn.Module):
    """Parameter container + 2D forward of a searched cell (skip_model_3d.py:12-75)."""

    def __init__(self, spec, cell_arch, steps, block_multiplier, dims):
        super().__init__()
        prims = PRIMITIVES_3D if dims == 3 else PRIMITIVES_2D
        self.spec = spec
        self.dims = dims
        self.c_out = spec.c_out
        self.steps = steps
        self.block_multiplier = block_multiplier
        self.downup_sample = spec.downup
        self.pre_preprocess = ConvBR(spec.c_prev_prev, spec.c_out, 1, 1, 0, dims=dims)
        self.preprocess = ConvBR(spec.c_prev, spec.c_out, 1, 1, 0, dims=dims)
        self._ops = nn.ModuleList()
        self.op_kinds = []
        for row in cell_arch:
            if prims[int(row[1])] == "skip_connect":
                self._ops.append(nn.Identity())
                self.op_kinds.append("skip")
            else:
                self._ops.append(ConvBR(spec.c_out, spec.c_out, 3, 1, 1, dims=dims))
                self.op_kinds.append("conv")
        self.plan = ops_in_iteration_order(np.asarray(cell_arch), steps)


def _head_modules(mod, initial_fm, dims, last3_bn_relu):
    mod.last_3 = ConvBR(initial_fm, 1 if dims == 3 else initial_fm, 3 if dims == 3 else 1, 1,
                        1 if dims == 3 else 0, bn=False, relu=False, dims=dims)
    mod.last_6 = ConvBR(initial_fm * 2, initial_fm, 1, 1, 0, dims=dims)
    mod.last_12 = ConvBR(initial_fm * 4, initial_fm * 2, 1, 1, 0, dims=dims)
    mod.last_24 = ConvBR(initial_fm * 8, initial_fm * 4, 1, 1, 0, dims=dims)


class _ExecutorCache:
    """Kernel-side parameters (packed weights, folded BN) built on first use and
    dropped whenever the weights may have changed: load_state_dict, .to(), and any
    in-place update of a parameter or buffer (an optimizer step, train-mode running
    statistics -- train.py alternates training with evaluation), seen through the
    tensors' version counters."""

    _executor_cls = None

    def invalidate(self):
        self._executor = None
        self._versioned = None

    def _weights_version(self):
        if getattr(self, "_versioned", None) is None:
            self._versioned = list(self.parameters()) + list(self.buffers())
        return sum(t._version for t in self._versioned)

    def _apply(self, fn, *a, **kw):
        self.invalidate()
        return super()._apply(fn, *a, **kw)

    def _load_from_state_dict(self, *a, **kw):
        self.invalidate()
        return super()._load_from_state_dict(*a, **kw)

    def executor(self):
        if self._executor is not None and self._executor_version != self._weights_version():
            self.invalidate()
        if self._executor is None:
            from . import executor
            self._executor = getattr(executor, self._executor_cls)(self)
            self._executor_version = self._weights_version()
        return self._executor


class NewFeature(_ExecutorCache, nn.Module):
    """2D feature net, retrain/new_model_2d.py:78-165, on the HIP kernels
    (``executor.FeatureExecutor``; ``FeatureExecutorBF16`` at precision bf16)."""

    _executor_cls = "FeatureExecutor"

    def set_precision(self, precision: str):
        cls = "FeatureExecutorBF16" if precision == "bf16" else "FeatureExecutor"
        if cls != self._executor_cls:
            self._executor_cls = cls
            self.invalidate()

    def __init__(self, network_arch, cell_arch, args):
        super().__init__()
        fm, bm, steps = args.fea_filter_multiplier, args.fea_block_multiplier, args.fea_step
        initial_fm = fm * bm
        self.cells = nn.ModuleList()  # registered first, as new_model_2d.py:82
        self.stem0 = ConvBR(3, initial_fm // 2, 3, stride=1, padding=1, dims=2)
        self.stem1 = ConvBR(initial_fm // 2, initial_fm, 3, stride=3, padding=1, dims=2)
        self.stem2 = ConvBR(initial_fm, initial_fm, 3, stride=1, padding=1, dims=2)
        specs = cell_specs(network_arch[: args.fea_num_layers], fm, bm)
        self.cells.extend(Cell(s, cell_arch, steps, bm, 2) for s in specs)
        _head_modules(self, initial_fm, 2, False)
        self._executor = None

    def forward(self, x, y=None):
        """newFeature.forward(x); with y, the features of x then y as one batch."""
        if not x.is_cuda:
            raise RuntimeError("leastereo_amd feature net runs on a ROCm device only")
        return self.executor().run(x, y)


class NewMatching(_ExecutorCache, nn.Module):
    """Matching net parameters (retrain/skip_model_3d.py:78-138); forward on HIP,
    in f32 (MatchingExecutor) or, with precision "bf16", on the bf16 engine
    (MatchingExecutorBF16, configs 3/4)."""

    _executor_cls = "MatchingExecutor"

    def set_precision(self, precision: str):
        """"f32", "bf16", or "f32_direct" (f32 on the direct-conv engine over the
        in-place cost volume: an independent algorithm, bench.py's per-pair check)."""
        cls = {"f32": "MatchingExecutor", "bf16": "MatchingExecutorBF16",
               "f32_direct": "MatchingExecutorDirect"}.get(precision)
        if cls is None:
            raise ValueError(f"precision must be 'f32', 'bf16' or 'f32_direct', got {precision!r}")
        if cls != self._executor_cls:
            self._executor_cls = cls
            self.invalidate()

    def __init__(self, network_arch, cell_arch, args):
        super().__init__()
        fm, bm, steps = args.mat_filter_multiplier, args.mat_block_multiplier, args.mat_step
        initial_fm = fm * bm
        self.cells = nn.ModuleList()  # registered first, as skip_model_3d.py:82
        self.stem0 = ConvBR(initial_fm * 2, initial_fm, 3, stride=1, padding=1)
        self.stem1 = ConvBR(initial_fm, initial_fm, 3, stride=1, padding=1)
        self.specs = cell_specs(network_arch[: args.mat_num_layers], fm, bm)
        self.cells.extend(Cell(s, cell_arch, steps, bm, 3) for s in self.specs)
        _head_modules(self, initial_fm, 3, False)
        self.conv1 = ConvBR(initial_fm * 4, initial_fm * 2, 3, 1, 1)
        self.conv2 = ConvBR(initial_fm * 4, initial_fm * 2, 3, 1, 1)
        self._executor = None

    def forward(self, cost):
        return self.executor().run(cost)


class Disp(nn.Module):
    """models/build_model_2d.py:45-57, fused into one HIP kernel."""

    def __init__(self, device, maxdisp=192):
        super().__init__()
        self.maxdisp = maxdisp
        self.device = device

    def forward(self, x, fast_exp=False):
        return kernels.disparity_regression(x, self.maxdisp, fast_exp)

    def stats(self, x, radius=4, fast_exp=False):
        """``forward`` plus the per-pixel entropy, peak mass and winner-window disparity of
        the same softmin distribution, in the same launch (``kernels.DisparityStats``)."""
        return kernels.disparity_regression_stats(x, self.maxdisp, radius, fast_exp)

    def right(self, x, fast_exp=False):
        """The right view's disparity from the same cost: the up-sampled cost read along its
        diagonals (``kernels.disparity_regression_right``)."""
        return kernels.disparity_regression_right(x, self.maxdisp, fast_exp)


class LEAStereo(nn.Module):
    """retrain/LEAStereo.py:12-52 with the hot path on MI355X kernels."""

    def __init__(self, args, device, precision=None):
        """``precision``: "f32" (default; the reference's arithmetic) or "bf16"
        (configs 3/4: matching net on bf16 activations with f32 accumulation; the
        feature net and the disparity regression stay f32).  Also read from
        ``args.precision`` when present."""
        super().__init__()
        network_path_fea = np.load(args.net_arch_fea)
        cell_arch_fea = np.load(args.cell_arch_fea)
        network_path_mat = np.load(args.net_arch_mat)
        cell_arch_mat = np.load(args.cell_arch_mat)
        self.maxdisp = args.maxdisp
        self.feature = NewFeature(network_layer_to_space(network_path_fea), cell_arch_fea, args)
        self.matching = NewMatching(network_layer_to_space(network_path_mat), cell_arch_mat, args)
        self.disp = Disp(device, self.maxdisp)
        self.use_cuda = getattr(args, "cuda", True)
        self.device = device
        self.precision = precision or getattr(args, "precision", None) or "f32"
        self.matching.set_precision(self.precision)
        self.feature.set_precision(self.precision)

    def check_shape(self, height: int, width: int):
        """Reject input sizes the reference cannot run."""
        # stem1 is k3/s3/p1 (new_model_2d.py:94): H3 = (H - 1) // 3 + 1
        check_matching_shape(int(self.maxdisp / 3), (height - 1) // 3 + 1, (width - 1) // 3 + 1,
                             self.matching.specs)

    def forward(self, x, y):
        if not x.is_cuda:
            raise RuntimeError("leastereo_amd.LEAStereo runs the matching net on a ROCm device only")
        self.check_shape(x.shape[2], x.shape[3])
        if self.training or (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)):
            # train.py:150-158: model.train(); model(input1, input2); loss.backward() -- the
            # differentiable path (train-mode BN, unfused op order, autograd through the
            # library's backward kernels); eval-mode inference takes the executors below
            from .training import leastereo_forward_train
            return leastereo_forward_train(self, x, y)
        # LEAStereo.py:31-32 runs the feature net twice; every layer is per-sample
        # (eval-mode BN), so one call on the stacked pair halves the launch count (the
        # fused stem reads x and y directly into the stacked stem1 maps)
        f = self.feature(x, y) if STEM_PAIR else self.feature(torch.cat((x, y), 0))
        fx, fy = f[: x.shape[0]], f[x.shape[0]:]
        # cost volume (:34-48) + matching (:50): stem0 reads the volume in place
        cost = self.matching.executor().run_features(fx, fy, self.maxdisp)
        return self.disp(cost, fast_exp=self.precision == "bf16")

    def forward_with_confidence(self, x, y, radius=4):
        """``forward`` that returns ``kernels.DisparityStats``: the same disparity (bit for
        bit) with the per-pixel entropy, peak mass and winner-window disparity of the head's
        softmin distribution (``DisparityStats.confidence``: 1 - entropy / ln maxdisp).
        Inference only: the outputs are not differentiable."""
        if not x.is_cuda:
            raise RuntimeError("leastereo_amd.LEAStereo runs the matching net on a ROCm device only")
        if self.training or (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)):
            raise RuntimeError("forward_with_confidence is inference only (its outputs have no backward): "
                               "call model.eval() and pass inputs that do not require grad")
        self.check_shape(x.shape[2], x.shape[3])
        f = self.feature(x, y) if STEM_PAIR else self.feature(torch.cat((x, y), 0))
        fx, fy = f[: x.shape[0]], f[x.shape[0]:]
        cost = self.matching.executor().run_features(fx, fy, self.maxdisp)
        return self.disp.stats(cost, radius, fast_exp=self.precision == "bf16")

    def forward_lr(self, x, y, threshold=1.0):
        """``forward`` with the left-right check, as ``kernels.DisparityLR``: the same disparity
        (bit for bit: the same feature, matching and head calls), the right view's disparity
        from the right head on the same cost (no second forward on the mirrored pair), the
        per-pixel state (``kernels.LR_CONSISTENT`` / ``LR_INCONSISTENT`` / ``LR_OUT_OF_VIEW``)
        and the scanline-filled disparity.  Inference only: the outputs are not differentiable."""
        if not x.is_cuda:
            raise RuntimeError("leastereo_amd.LEAStereo runs the matching net on a ROCm device only")
        if self.training or (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)):
            raise RuntimeError("forward_lr is inference only (its outputs have no backward): "
                               "call model.eval() and pass inputs that do not require grad")
        self.check_shape(x.shape[2], x.shape[3])
        f = self.feature(x, y) if STEM_PAIR else self.feature(torch.cat((x, y), 0))
        fx, fy = f[: x.shape[0]], f[x.shape[0]:]
        cost = self.matching.executor().run_features(fx, fy, self.maxdisp)
        fast = self.precision == "bf16"
        disp = self.disp(cost, fast_exp=fast)
        return kernels.lr_check(disp, self.disp.right(cost, fast_exp=fast), threshold)

    def forward_refined(self, x, y, lam=kernels.REFINE_LAMBDA, sigma=kernels.REFINE_SIGMA,
                        iterations=kernels.REFINE_ITERATIONS, radius=4, lr_threshold=1.0, speckle=None):
        """``forward`` with the confidence-weighted edge-preserving refinement, as
        ``kernels.DisparityRefined``: one feature call, one matching call, the stats head (the
        disparity of ``forward`` bit for bit, and the peak mass within ``radius``), the right
        head, the left-right check at ``lr_threshold``, then ``kernels.fgs_refine`` with the
        left image ``x`` as guide, ``conf`` the peak mass and ``exclude`` the check's state.
        ``sigma`` is in units of the standardised image that ``forward`` receives; the defaults
        restate OpenCV's and are untuned.  ``speckle=dict(max_size=..., max_diff=...)`` (an empty
        dict for the untuned defaults of ``kernels.speckle_filter``) runs the speckle filter
        between the check and the refinement, as OpenCV does: on the disparity, with the check's
        flags as walls; the refinement then excludes, and so fills, the removed components too,
        and ``state`` marks them ``kernels.LR_SPECKLE``.  ``None``: no such call.
        Inference only: the outputs are not differentiable."""
        if not x.is_cuda:
            raise RuntimeError("leastereo_amd.LEAStereo runs the matching net on a ROCm device only")
        if self.training or (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)):
            raise RuntimeError("forward_refined is inference only (its outputs have no backward): "
                               "call model.eval() and pass inputs that do not require grad")
        if speckle is not None and (not isinstance(speckle, dict) or set(speckle) - {"max_size", "max_diff"}):
            raise ValueError(f"forward_refined: speckle must be None or a dict of max_size / max_diff, got {speckle!r}")
        self.check_shape(x.shape[2], x.shape[3])
        f = self.feature(x, y) if STEM_PAIR else self.feature(torch.cat((x, y), 0))
        fx, fy = f[: x.shape[0]], f[x.shape[0]:]
        cost = self.matching.executor().run_features(fx, fy, self.maxdisp)
        fast = self.precision == "bf16"
        st = self.disp.stats(cost, radius, fast_exp=fast)  # the call of forward_with_confidence
        lr = kernels.lr_check(st.disp, self.disp.right(cost, fast_exp=fast), lr_threshold, want_filled=False)
        state = lr.state
        if speckle is not None:
            state = kernels.speckle_filter(st.disp, state, want_size=False, want_filtered=False, **speckle).state
        refined, support = kernels.fgs_refine(x, st.disp, st.peak, state, lam, sigma, iterations,
                                              return_support=True)
        return kernels.DisparityRefined(st.disp, refined, support, st.peak, lr.disp_right, state)

    _POINT_OPTS = ("min_disp", "max_disp", "normals", "normal_max_diff", "capacity", "want_points", "want_valid",
                   "want_compact")

    def forward_points(self, x, y, Q, image=None, refine=True, **opts):
        """``forward_refined`` with the point cloud as the last stage, as
        (``kernels.DisparityRefined``, ``kernels.PointCloud``): the chain of ``forward_refined``
        (its keywords in ``opts``: lam, sigma, iterations, radius, lr_threshold, speckle), then
        ``kernels.reproject`` of ``disp_refined`` through ``Q`` with ``exclude`` the chain's
        ``state`` (the keywords of ``reproject`` in ``opts``: min_disp, max_disp, normals,
        normal_max_diff, capacity, want_points, want_valid, want_compact).  ``refine=False``
        reprojects the plain disparity ``disp`` instead.  ``image``: the uint8 left image
        [B, H, W, 3|4] on the device, for the colours.  ``Q`` as for ``reproject``: a float32
        device tensor is read in place.  Nothing is read back.  Inference only."""
        pc = {k: opts.pop(k) for k in self._POINT_OPTS if k in opts}
        out = self.forward_refined(x, y, **opts)
        cloud = kernels.reproject(out.disp_refined if refine else out.disp, Q, image, out.state, **pc)
        return out, cloud

    def forward_scene(self, left_u8, right_u8, tile, **kw):
        """A uint8 scene pair [H, W, 3|4] of any size through overlapping ``tile`` = (h, w)
        forwards, gathered and blended on the device: ``scene.SceneResult`` at the scene's
        size.  ``kw`` as ``scene.SceneRunner`` (tile_batch, context, ramp, confidence, radius,
        lr_threshold, graph); the runners (their captured graphs and tile plans) are kept per
        setting.  Inference only."""
        from .scene import SceneRunner
        key = (int(tile[0]), int(tile[1]), tuple(sorted(kw.items())))
        runners = self.__dict__.setdefault("_scene_runners", {})
        if key not in runners:
            runners[key] = SceneRunner(self, key[0], key[1], **kw)
        return runners[key](left_u8, right_u8)

    def set_precision(self, precision: str):
        """Switch the arithmetic ("f32" / "bf16" / "f32_direct"); weights are re-packed
        on the next forward."""
        self.matching.set_precision(precision)
        self.feature.set_precision(precision)
        self.precision = precision

    def graphed(self, batch: int, height: int, width: int, confidence: bool = False, radius: int = 4,
                lr_threshold=None, refine=None, points=None):
        """``forward`` for one input shape captured into a HIP graph (SURVEY.md §7:
        one host call per batch instead of ~140 launches, for serving and for ranks
        that share a node's host CPUs).  The forward issues only library kernels on
        the current stream and never synchronises, so it captures as is.
        ``confidence=True`` captures ``forward_with_confidence(..., radius)`` instead, a number
        for ``lr_threshold`` captures ``forward_lr(..., lr_threshold)``; not both in one capture.
        ``refine=dict(...)`` (the keywords of ``forward_refined``, ``speckle=dict(...)`` among them;
        an empty dict for its defaults) captures ``forward_refined`` instead, on its own.
        ``points=dict(Q=..., ...)`` (the other keywords of ``forward_points``: refine=False,
        image=True for a static uint8 [B, H, W, 3] colour buffer, and those of
        ``kernels.reproject``) captures ``forward_points`` with the ``refine`` dict's chain: the
        output is (``DisparityRefined``, ``PointCloud``), and every replay reads the matrix the
        captured device tensor ``.Q`` holds at the time (``__call__(x, y, Q=new)`` copies into it)."""
        return GraphedForward(self, batch, height, width, confidence, radius, lr_threshold, refine, points)


class GraphedForward:
    """``forward`` captured once into a torch.cuda.CUDAGraph (a hipGraph on ROCm)
    with static input/output buffers; ``__call__(x, y)`` copies the inputs in,
    replays, and returns the static output (overwritten by the next call): the disparity,
    with ``confidence`` the ``DisparityStats`` of ``forward_with_confidence``, or with
    ``lr_threshold`` the ``DisparityLR`` of ``forward_lr``, or with ``refine`` the
    ``DisparityRefined`` of ``forward_refined``, or with ``points`` the (``DisparityRefined``,
    ``PointCloud``) of ``forward_points``: its matrix is the static device tensor ``Q`` ([4, 4]
    or [B, 4, 4] float32), its colours the static uint8 ``image`` [B, H, W, 3] (``None`` without
    ``image=True``); ``__call__(x, y, Q=None, image=None)`` copies into them what it is given."""

    def __init__(self, model: LEAStereo, batch: int, height: int, width: int, confidence: bool = False,
                 radius: int = 4, lr_threshold=None, refine=None, points=None):
        if points is not None:
            if not isinstance(points, dict) or "Q" not in points:
                raise ValueError(f"graphed(): points must be a dict with the matrix Q, got {points!r}")
            refine = {} if refine is None else refine
        if refine is not None and (confidence or lr_threshold is not None):
            raise ValueError("graphed(): refine=dict(...) captures forward_refined on its own; give radius and "
                             "lr_threshold inside the dict")
        if confidence and lr_threshold is not None:
            raise ValueError("graphed(): confidence=True and lr_threshold in one capture is not supported; "
                             "capture two graphs")
        if not torch.cuda.is_available():
            raise RuntimeError("HIP graphs need a ROCm device")
        if model.training:
            # a train-mode forward is the differentiable path (batch-statistics BN, running
            # statistics updated per call, autograd buffers): capture inference only
            raise RuntimeError("graphed() captures the eval-mode forward: call model.eval() first")
        model.check_shape(height, width)
        dev = next(model.parameters()).device
        self.model = model
        self.Q = self.image = None
        if points is not None:
            pc = dict(points)
            self.Q = kernels._as_q(pc.pop("Q"), batch, dev).clone()
            if pc.pop("image", False):
                self.image = torch.zeros(batch, height, width, 3, device=dev, dtype=torch.uint8)
            pc.update(refine)
        run = ((lambda a, b: model.forward_points(a, b, self.Q, self.image, **pc)) if points is not None else
               (lambda a, b: model.forward_refined(a, b, **refine)) if refine is not None else
               (lambda a, b: model.forward_with_confidence(a, b, radius)) if confidence else
               (lambda a, b: model.forward_lr(a, b, lr_threshold)) if lr_threshold is not None else model)
        self.x = torch.zeros(batch, 3, height, width, device=dev)
        self.y = torch.zeros_like(self.x)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(2):  # packs the weights and warms the allocator outside the capture
                run(self.x, self.y)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = run(self.x, self.y)

    def __call__(self, x, y, Q=None, image=None):
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)
        if Q is not None or image is not None:
            if self.Q is None or (image is not None and self.image is None):
                raise ValueError("GraphedForward: Q and image go with graphed(points=dict(Q=..., image=True))")
            if Q is not None:
                self.Q.copy_(kernels._as_q(Q, self.x.shape[0], self.Q.device).reshape(self.Q.shape), non_blocking=True)
            if image is not None:
                self.image.copy_(image[..., :3], non_blocking=True)
        self.graph.replay()
        return self.out
