"""Tensor-level wrappers over the C ABI: device tensors in, device tensors out.

Each wrapper checks shapes/strides on the host, then launches on the current
HIP stream (``torch.cuda.current_stream()``), so it composes with torch ops
and is capturable by ``torch.cuda.graph``.  There is no fallback: a non-CUDA
tensor or a missing library raises.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import LEA_BF16, LEA_CVS_TMAJOR, LEA_F32, LEA_PAIR_SUM, LEA_RELU, LEA_RESIDUAL, check


def _stream():
    return torch.cuda.current_stream().cuda_stream


# one launch's probe record; positional use (r[0], r[2], r[6]) is part of the interface
ProbeRecord = collections.namedtuple("ProbeRecord", "name flops bytes start end mfma_flops shape")


class KernelProbe:
    """Times launches of conv kernel instantiations with HIP events recorded on
    the stream the kernel is launched on (torch's current stream).

    ``names=None`` records every conv launch.  Each record carries the launch's
    algorithmic FLOPs and bytes (input + output + weights [+ residual read]).
    """

    def __init__(self, names=None):
        self.names = None if names is None else set(names)
        self.records = []  # ProbeRecord(name, flops, bytes, start_event, end_event, mfma_flops, shape)

    def __enter__(self):
        global _probe
        _probe = self
        return self

    def __exit__(self, *exc):
        global _probe
        _probe = None

    def _totals(self, key, name=None):
        torch.cuda.synchronize()
        out = {}
        for r in self.records:
            if name is not None and r.name != name:
                continue
            d = out.setdefault(key(r), {"launches": 0, "flops": 0.0, "bytes": 0.0, "ms": 0.0, "mfma_flops": 0.0})
            d["launches"] += 1
            d["flops"] += r.flops
            d["bytes"] += r.bytes
            d["ms"] += r.start.elapsed_time(r.end)
            d["mfma_flops"] += r.mfma_flops
        return out

    def summary(self):
        return self._totals(lambda r: r.name)

    def by_shape(self, name):
        """Launches of kernel ``name`` grouped by layer shape (B, cin, cout, D, H, W, k)."""
        return self._totals(lambda r: r.shape, name)


_probe = None


def _conv_record(b, cin, cout, d, h, w, k, accumulate, in_vox, resampled, name=None, mfma_scale=1.0,
                 esz=4, nbytes=None):
    """The probe record of a 3D conv launch, or None if the active probe does not want its kernel.
    ``flops`` is the direct convolution's (the reference algorithm's) count;
    ``mfma_scale`` converts it to the products the kernel actually issues (2/3 for
    Winograd F(2,3), times its cout padding); ``esz`` is the activation element size;
    ``nbytes`` replaces the algorithmic byte count (input + output [+ residual] + weights)."""
    if name is None:
        name = conv_kernel_name(b, cout, d, h, w, k, resampled, cin)
    if _probe.names is not None and name not in _probe.names:
        return None
    vox = b * d * h * w
    flops = 2.0 * vox * cout * cin * k ** 3
    if nbytes is None:
        nbytes = esz * (in_vox * cin + vox * cout * (2 if accumulate else 1)) + 4.0 * cout * cin * k ** 3
    return ProbeRecord(name, flops, nbytes, None, None, flops * mfma_scale, (b, cin, cout, d, h, w, k))


def _op_record(name, flops, nbytes, mfma=None, shape=None):
    """The probe record of a launch that is not a 3D conv (2D convs, resamples, the head, the
    disparity regression, layout conversions), or None if the active probe does not want it:
    ``flops`` / ``nbytes`` are its algorithmic work, ``mfma`` the matrix-core products it issues
    (default: flops)."""
    if _probe.names is not None and name not in _probe.names:
        return None
    return ProbeRecord(name, float(flops), float(nbytes), None, None, float(flops if mfma is None else mfma), shape)


@contextlib.contextmanager
def _timed(record):
    """HIP-event timing of what the block launches, as one record of the active probe.  ``record``
    is a callable that returns the launch's ``_conv_record`` / ``_op_record``; it is called only
    while a KernelProbe is active, so without one a launch costs no event, no kernel-name query
    and no arithmetic.  A block that raises records nothing."""
    probe = _probe
    rec = None if probe is None or record is None else record()
    if rec is None:
        yield
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    yield
    e1.record()
    probe.records.append(rec._replace(start=e0, end=e1))


def _call(entry, *args):
    """The return code of library entry point ``entry`` (a key of ``_lib.SIGNATURES``) called with
    ``args`` and, last, the current stream."""
    return getattr(_lib.load(), entry)(*args, _stream())


def _launch(entry, *args, probe=None):
    """Launch ``entry`` on the current stream and raise on failure; ``probe``: see ``_timed``."""
    if _probe is None or probe is None:
        check(_call(entry, *args), entry)
    else:
        with _timed(probe):
            check(_call(entry, *args), entry)


# ---- operand checks shared by the wrappers ----

def _ptr(t):
    return None if t is None else t.data_ptr()


def _contiguous(t):
    return None if t is None else t.contiguous()


def _decode(name):
    return name.decode() if name else None


def _flags(relu, residual=False, pair_sum=False):
    return (LEA_RELU if relu else 0) | (LEA_RESIDUAL if residual else 0) | (LEA_PAIR_SUM if pair_sum else 0)


def _require_cuda(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise _lib.HipKernelError(
                f"HIP path needs float32 tensors on a ROCm device, got {t.dtype} on {t.device}")


def _check_volume_view(t: torch.Tensor, name: str):
    """NCDHW tensor whose (C, D, H, W) block is contiguous per batch (a channel
    slice of a contiguous tensor qualifies); returns the batch stride."""
    b, c, d, h, w = t.shape
    if t.stride()[1:] != (d * h * w, h * w, w, 1):
        raise ValueError(f"{name}: NCDHW slice with contiguous C,D,H,W required, strides {t.stride()}")
    return t.stride(0)


def _f32_volume(t, aligned):
    """Whether ``t`` is an f32 NCDHW device tensor with contiguous C,D,H,W, with ``aligned`` also
    16-byte aligned with batch strides of whole 16-byte words (the ``*_supported`` queries)."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 5:
        return False
    d, h, w = t.shape[2:]
    if aligned and (t.data_ptr() % 16 or t.stride(0) % 4):
        return False
    return t.stride()[1:] == (d * h * w, h * w, w, 1)


def _number(who, name, v, want, lo=None, hi=None, finite=False, integer=False, bools=False):
    """ValueError ``who: name v must be want`` unless ``v`` is an int or float (an int with
    ``integer``; a bool only with ``bools``), finite with ``finite``, and, given bounds,
    lo <= v <= hi (which no NaN passes; ``lo=-inf`` is the check for NaN alone)."""
    ok = isinstance(v, int if integer else (int, float)) and (bools or not isinstance(v, bool))
    if ok and lo is not None:
        ok = lo <= v <= (math.inf if hi is None else hi)
    if not ok or (finite and not math.isfinite(v)):
        raise ValueError(f"{who}: {name} {v} must be {want}")


def _exclude_u8(exclude, shape, who=None):
    """The exclude mask of the disparity post-processing: None, or a uint8 or bool device tensor
    of ``shape``, returned as uint8 (a view; the caller makes it contiguous where it stages its
    operands).  ``who`` prefixes the message and names the shape."""
    if exclude is None:
        return None
    if (not isinstance(exclude, torch.Tensor) or not exclude.is_cuda or tuple(exclude.shape) != shape
            or exclude.dtype not in (torch.uint8, torch.bool)):
        raise ValueError("exclude must be a [B, H, W] uint8 or bool tensor on the device" if who is None else
                         f"{who}: exclude must be a {shape} uint8 or bool tensor on the device")
    return exclude.view(torch.uint8) if exclude.dtype == torch.bool else exclude


def _as_f32(a, device, what) -> torch.Tensor:
    """An array or tensor as a contiguous float32 tensor on the device; one that is that already
    is used in place.  ``what`` opens the message for one that is not floating point."""
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).astype(np.float32))
    if not a.dtype.is_floating_point:
        raise ValueError(f"{what}, got {a.dtype}")
    return a.to(device=device, dtype=torch.float32).contiguous()


def _feature_pair(fl, fr):
    """The two feature maps of a cost-volume conv, read in place: returns (B, C, H, W)."""
    if fl.shape != fr.shape or fl.dim() != 4:
        raise ValueError("left/right features must both be [B, C, H, W]")
    if fl.stride() != fr.stride() or fl.stride()[1:] != (fl.shape[2] * fl.shape[3], fl.shape[3], 1):
        raise ValueError("left/right features need contiguous C,H,W and equal strides")
    return fl.shape


def _head_cost(cost):
    """The matching cost of the disparity heads, contiguous, and its (B, D3, H3, W3)."""
    _require_cuda(cost)
    if cost.dim() != 5 or cost.shape[1] != 1:
        raise ValueError("cost must be [B, 1, D3, H3, W3]")
    cost = cost.contiguous()
    b, _, d3, h3, w3 = cost.shape
    return cost, b, d3, h3, w3


def _sums_scales(sums, scales, of, parts):
    """The backward operands of the two losses: ``sums`` as ``of`` returned it, ``scales`` two
    float32 (``parts``) on the device."""
    _require_cuda(scales)
    if not sums.is_cuda or sums.dtype != torch.float64 or sums.numel() != 4 or not sums.is_contiguous():
        raise ValueError(f"sums: the contiguous float64 [4] device tensor of {of}")
    if scales.numel() != 2 or not scales.is_contiguous():
        raise ValueError(f"scales: two contiguous float32 ({parts}) on the device")


# Activation layouts: f32 NCDHW [B, C, D, H, W], or bf16 "c8" [B, C/8, D, H, W, 8] (8 channels per
# voxel word); the helpers below take ``c8`` to choose.

def _require_c8(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 6
                              or t.shape[-1] != 8):
            raise _lib.HipKernelError(
                f"bf16 path needs [B, C/8, D, H, W, 8] bfloat16 ROCm tensors, got {t.dtype} "
                f"{tuple(t.shape)} on {t.device}")


def _check_c8_view(t: torch.Tensor, name: str):
    b, cb, d, h, w, _ = t.shape
    if t.stride()[1:] != (d * h * w * 8, h * w * 8, w * 8, 8, 1):
        raise ValueError(f"{name}: c8 block slice with contiguous blocks required, strides {t.stride()}")
    return t.stride(0)


def _batch_stride(t, name, c8=False):
    return _check_c8_view(t, name) if c8 else _check_volume_view(t, name)


def _act_shape(b, c, spatial, c8=False):
    spatial = tuple(int(s) for s in spatial)
    return (b, c // 8) + spatial + (8,) if c8 else (b, c) + spatial


def _out_view(t, shape, device, c8=False, name="out"):
    """``t``, or with None a new tensor, of ``shape`` in the layout (``t`` may be a channel slice
    of a larger tensor); returns it and its batch stride."""
    if t is None:
        t = torch.empty(shape, device=device, dtype=torch.bfloat16 if c8 else torch.float32)
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} shape {tuple(t.shape)} != {shape}")
    return t, _batch_stride(t, name, c8)


def _conv_out(b, cout, spatial, out, accumulate, device, c8=False):
    if out is None and accumulate:
        raise ValueError("accumulate needs out")
    return _out_view(out, _act_shape(b, cout, spatial, c8), device, c8)


def _residual(out, accumulate, residual, ybs, c8=False, shape=None):
    """(pointer, batch stride) of the epilogue's residual: ``out`` itself under
    ``accumulate``, else an explicit tensor of out's shape (``shape`` where there is no out),
    or none."""
    if accumulate:
        if residual is not None:
            raise ValueError("accumulate and residual are exclusive")
        return out.data_ptr(), ybs
    if residual is None:
        return None, 0
    (_require_c8 if c8 else _require_cuda)(residual)
    shape = tuple(out.shape) if shape is None else shape
    if tuple(residual.shape) != shape:
        raise ValueError(f"residual shape {tuple(residual.shape)} != {shape}")
    return residual.data_ptr(), _batch_stride(residual, "residual", c8)


def _second_source(x2, b, spatial, c8=False):
    """(pointer, batch stride, channels) of a conv's optional second source, read as
    ``torch.cat((x, x2), 1)`` without the copy; (None, 0, 0) without one."""
    if x2 is None:
        return None, 0, 0
    if x2.shape[0] != b or tuple(x2.shape[2:5]) != spatial:
        raise ValueError("x2 must match x in batch and volume")
    return x2.data_ptr(), _batch_stride(x2, "x2", c8), x2.shape[1] * (8 if c8 else 1)


def conv_kernel_name(b, cout, d, h, w, k, resampled=False, cin=None):
    """The kernel of an f32 conv launch; without ``cin``, of one with at most 128 input channels
    (a wider resampled 1x1 runs on the register-staged engine)."""
    if cin is None:
        return _decode(_lib.load().lea_conv3d_kernel_name(b, cout, d, h, w, k, 1 if resampled else 0))
    return _decode(_lib.load().lea_conv3d_launch_kernel_name(b, cin, 0, cout, d, h, w, k, 1 if resampled else 0))


def build_cost_volume(fl: torch.Tensor, fr: torch.Tensor, maxdisp: int) -> torch.Tensor:
    """retrain/LEAStereo.py:34-48 -> [B, 2C, int(maxdisp/3), H, W]."""
    _require_cuda(fl, fr)
    fl, fr = fl.contiguous(), fr.contiguous()
    if fl.shape != fr.shape or fl.dim() != 4:
        raise ValueError("left/right features must both be [B, C, H, W]")
    b, c, h, w = fl.shape
    d3 = int(maxdisp / 3)
    cost = torch.empty((b, 2 * c, d3, h, w), device=fl.device, dtype=fl.dtype)
    _launch("lea_build_cost_volume", fl.data_ptr(), fr.data_ptr(), cost.data_ptr(), b, c, h, w, d3, LEA_F32)
    return cost


def packed_floats(cout: int, cin: int, k: int) -> int:
    n = _lib.load().lea_conv3d_packed_floats(cout, cin, k)
    if n == 0:
        raise ValueError(f"unsupported conv shape cout={cout} cin={cin} k={k}")
    return n


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[cout, cin, k, k, k] fp32 device weight -> the kernel's packed layout."""
    _require_cuda(w)
    w = w.detach().contiguous()
    cout, cin, k = w.shape[0], w.shape[1], w.shape[-1]
    packed = torch.empty(packed_floats(cout, cin, k), device=w.device, dtype=torch.float32)
    _launch("lea_conv3d_pack_weights", w.data_ptr(), packed.data_ptr(), cout, cin, k)
    return packed


def conv3d_bnrelu(x: torch.Tensor, packed: torch.Tensor, cout: int, k: int,
                  scale: torch.Tensor | None, shift: torch.Tensor | None, relu: bool = True,
                  out: torch.Tensor | None = None, accumulate: bool = False,
                  x2: torch.Tensor | None = None,
                  residual: torch.Tensor | None = None) -> torch.Tensor:
    """ConvBR3d (operations_3d.py:41-47) of ``torch.cat((x, x2), 1)`` (x2 optional,
    never materialised).  ``out`` may be a channel slice of a larger (cat) buffer;
    ``accumulate`` adds the activation to what ``out`` holds (the cell's pairwise
    sum, skip_model_3d.py:69)."""
    _require_cuda(x, x2, packed, scale, shift, out)
    b, cin, d, h, w = x.shape
    xbs = _check_volume_view(x, "x")
    x2ptr, x2bs, cin2 = _second_source(x2, b, (d, h, w))
    out, ybs = _conv_out(b, cout, (d, h, w), out, accumulate, x.device)
    rptr, rbs = _residual(out, accumulate, residual, ybs)
    _launch("lea_conv3d_bnrelu", x.data_ptr(), xbs, x2ptr, x2bs, cin2, packed.data_ptr(), _ptr(scale),
            _ptr(shift), rptr, rbs, out.data_ptr(), ybs, b, cin + cin2, cout, d, h, w, k,
            _flags(relu, rptr is not None), LEA_F32,
            probe=lambda: _conv_record(b, cin + cin2, cout, d, h, w, k, rptr is not None, b * d * h * w, False))
    return out


def conv1x1_heads(x: torch.Tensor, packed: torch.Tensor, cout_a: int, scale_a, shift_a, relu_a: bool,
                  cout_b: int, scale_b, shift_b, relu_b: bool, out_a: torch.Tensor | None = None,
                  out_b: torch.Tensor | None = None, x2: torch.Tensor | None = None,
                  accumulate: bool = False, residual: torch.Tensor | None = None):
    """Two 1x1 ConvBR3d of ``torch.cat((x, x2), 1)`` over one read of it (lea_conv1x1_heads):
    ``packed`` is ``pack_conv_weight`` of the two weights stacked along cout, head A's first; each
    head has its own folded BN (None: none), ReLU and output (a channel slice of a larger buffer
    qualifies).  Returns (out_a, out_b), each bit-identical to its own ``conv3d_bnrelu(k=1)``.
    Neither head accumulates or takes a residual."""
    if accumulate or residual is not None:
        raise ValueError("conv1x1_heads: neither head accumulates or takes a residual")
    _require_cuda(x, x2, packed, scale_a, shift_a, scale_b, shift_b, out_a, out_b)
    b, cin, d, h, w = x.shape
    xbs = _check_volume_view(x, "x")
    x2ptr, x2bs, cin2 = _second_source(x2, b, (d, h, w))
    out_a, abs_ = _out_view(out_a, _act_shape(b, cout_a, (d, h, w)), x.device, name="out_a")
    out_b, bbs = _out_view(out_b, _act_shape(b, cout_b, (d, h, w)), x.device, name="out_b")
    cout = cout_a + cout_b
    _launch("lea_conv1x1_heads", x.data_ptr(), xbs, x2ptr, x2bs, cin2, packed.data_ptr(),
            _ptr(scale_a), _ptr(shift_a), out_a.data_ptr(), abs_, cout_a, _flags(relu_a),
            _ptr(scale_b), _ptr(shift_b), out_b.data_ptr(), bbs, cout_b, _flags(relu_b),
            b, cin + cin2, d, h, w, LEA_F32,
            probe=lambda: _conv_record(b, cin + cin2, cout, d, h, w, 1, False, b * d * h * w, False,
                                       name=_decode(_lib.load().lea_conv1x1_heads_kernel_name(b, cout, d, h, w))))
    return out_a, out_b


def costvolume_kernel_name(b, cout, d3, h, w):
    return _decode(_lib.load().lea_conv3d_costvolume_kernel_name(b, cout, d3, h, w))


def conv3d_bnrelu_costvolume(fl: torch.Tensor, fr: torch.Tensor, maxdisp: int, packed: torch.Tensor,
                             cout: int, scale: torch.Tensor | None, shift: torch.Tensor | None,
                             relu: bool = True) -> torch.Tensor:
    """ConvBR3d 3x3x3 of the cost volume of (fl, fr) (LEAStereo.py:34-48 then
    skip_model_3d.py:141) without materialising the volume; bit-identical to
    ``conv3d_bnrelu(build_cost_volume(fl, fr, maxdisp), ...)``."""
    _require_cuda(fl, fr, packed, scale, shift)
    b, c, h, w = _feature_pair(fl, fr)
    d3 = int(maxdisp / 3)
    out = torch.empty((b, cout, d3, h, w), device=fl.device, dtype=fl.dtype)
    _launch("lea_conv3d_bnrelu_costvolume", fl.data_ptr(), fr.data_ptr(), fl.stride(0), packed.data_ptr(),
            _ptr(scale), _ptr(shift), out.data_ptr(), out.stride(0), b, c, cout, d3, h, w, _flags(relu), LEA_F32,
            probe=lambda: _conv_record(b, 2 * c, cout, d3, h, w, 3, False, 0, False,
                                       name=costvolume_kernel_name(b, cout, d3, h, w)))
    return out


def conv3d_bnrelu_resampled(x: torch.Tensor, size, packed: torch.Tensor, cout: int, k: int,
                            scale: torch.Tensor | None, shift: torch.Tensor | None,
                            relu: bool = True, out: torch.Tensor | None = None,
                            accumulate: bool = False) -> torch.Tensor:
    """ConvBR3d(F.interpolate(x, size, mode='trilinear', align_corners=True)) with
    the interpolation fused into the conv's input staging (skip_model_3d.py:44-53)."""
    _require_cuda(x, packed, scale, shift, out)
    b, cin, di, hi, wi = x.shape
    d, h, w = (int(s) for s in size)
    xbs = _check_volume_view(x, "x")
    out, ybs = _conv_out(b, cout, (d, h, w), out, accumulate, x.device)
    rptr, rbs = _residual(out, accumulate, None, ybs)
    _launch("lea_conv3d_bnrelu_resampled", x.data_ptr(), xbs, di, hi, wi, packed.data_ptr(), _ptr(scale),
            _ptr(shift), rptr, rbs, out.data_ptr(), ybs, b, cin, cout, d, h, w, k, _flags(relu, accumulate),
            LEA_F32,
            probe=lambda: _conv_record(b, cin, cout, d, h, w, k, accumulate, b * di * hi * wi, True))
    return out


# ------------------------------------------------------------------- 2D feature net
# Feature-net activations travel as NCDHW views with D = 1 ([B, C, 1, H, W]), so the
# 1x1 convs and bilinear resizes are the 3D entry points on a single plane.

def conv2d_kernel_name(b, cout, h, w, cin=None):
    lib = _lib.load()
    return _decode(lib.lea_conv2d_kernel_name(b, cout, h, w) if cin is None
                   else lib.lea_conv2d_kernel_name_cin(b, cin, cout, h, w))


def _conv2d_weight(w):
    """A [cout, cin, 3, 3] f32 device weight, contiguous, with its cout and cin."""
    _require_cuda(w)
    w = w.detach().contiguous()
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"expected a [cout, cin, 3, 3] weight, got {tuple(w.shape)}")
    return w, w.shape[0], w.shape[1]


def pack_conv2d_weight(w: torch.Tensor) -> torch.Tensor:
    """[cout, cin, 3, 3] fp32 device weight -> packed layout of lea_conv2d_bnrelu."""
    w, cout, cin = _conv2d_weight(w)
    n = _lib.load().lea_conv2d_packed_floats(cout, cin)
    packed = torch.empty(n, device=w.device, dtype=torch.float32)
    _launch("lea_conv2d_pack_weights", w.data_ptr(), packed.data_ptr(), cout, cin)
    return packed


def conv2d_bnrelu(x: torch.Tensor, packed: torch.Tensor, cout: int,
                  scale: torch.Tensor | None, shift: torch.Tensor | None, relu: bool = True,
                  out: torch.Tensor | None = None, accumulate: bool = False,
                  residual: torch.Tensor | None = None) -> torch.Tensor:
    """ConvBR2d 3x3/s1/p1 (operations_2d.py:31-47) on x [B, cin, 1, H, W]; ``residual``
    (or ``accumulate`` into out) adds a cell-sum operand in the epilogue."""
    _require_cuda(x, packed, scale, shift, out)
    b, cin, d, h, w = x.shape
    if d != 1:
        raise ValueError("conv2d_bnrelu takes [B, C, 1, H, W] views")
    xbs = _check_volume_view(x, "x")
    out, ybs = _conv_out(b, cout, (1, h, w), out, accumulate, x.device)
    rptr, rbs = _residual(out, accumulate, residual, ybs)
    _launch("lea_conv2d_bnrelu", x.data_ptr(), xbs, packed.data_ptr(), _ptr(scale), _ptr(shift), rptr, rbs,
            out.data_ptr(), ybs, b, cin, cout, h, w, _flags(relu, rptr is not None), LEA_F32,
            probe=lambda: _op_record(
                conv2d_kernel_name(b, cout, h, w, cin), 2.0 * b * h * w * cout * cin * 9,
                4.0 * b * h * w * (cin + cout * (2 if rptr is not None else 1)) + 36.0 * cout * cin))
    return out


def pack_conv2d_weight_windowed(w: torch.Tensor, split: int) -> torch.Tensor:
    """The packed weight of ``conv2d_bnrelu_windowed``: rows [0, split) and rows [split, cout) of a
    [cout, cin, 3, 3] weight, each packed as ``pack_conv2d_weight`` does, one after the other."""
    w, cout, _ = _conv2d_weight(w)
    if not 0 <= split < cout:
        raise ValueError(f"split {split} must be in [0, {cout})")
    return torch.cat([pack_conv2d_weight(part) for part in (w[:split], w[split:]) if part.shape[0]])


def conv2d_windowed_tiles(w: int, windows):
    """The windows of ``conv2d_bnrelu_windowed`` as it runs them, in 16-column tiles:
    [(begin, end), ...] -- rounded outward, merged where they touch."""
    w1, w2 = (tuple(windows) + ((0, 0),))[:2]
    t = (ctypes.c_int * 4)()
    check(_lib.load().lea_conv2d_windowed_tiles(w, w1[0], w1[1], w2[0], w2[1], t), "lea_conv2d_windowed_tiles")
    return [(t[i], t[i + 1]) for i in (0, 2) if t[i] < t[i + 1]]


def conv2d_bnrelu_windowed(x: torch.Tensor, packed: torch.Tensor, cout: int, split: int, windows,
                           scale: torch.Tensor | None = None, shift: torch.Tensor | None = None,
                           relu: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """``conv2d_bnrelu`` on the direct engine with output channels [0, split) computed on every
    column and channels [split, cout) only on the columns of ``windows`` (one or two (begin, end),
    rounded outward to 16-column tiles); nothing else of ``out`` is written
    (lea_conv2d_bnrelu_windowed).  ``packed``: ``pack_conv2d_weight_windowed``."""
    _require_cuda(x, packed, scale, shift, out)
    b, cin, d, h, w = x.shape
    if d != 1:
        raise ValueError("conv2d_bnrelu_windowed takes [B, C, 1, H, W] views")
    xbs = _check_volume_view(x, "x")
    out, ybs = _conv_out(b, cout, (1, h, w), out, False, x.device)
    w1, w2 = (tuple(windows) + ((0, 0),))[:2]
    cols = sum(16 * (e - s) for s, e in conv2d_windowed_tiles(w, windows))

    def record():
        px = b * h * (split * w + (cout - split) * min(cols, w))  # output values computed
        return _op_record(conv2d_kernel_name(b, cout - split, h, w, None) + " windowed", 2.0 * px * cin * 9,
                          4.0 * (b * h * w * cin + px) + 36.0 * cout * cin, shape=(b, cin, cout, 1, h, w, 3))
    _launch("lea_conv2d_bnrelu_windowed", x.data_ptr(), xbs, packed.data_ptr(), _ptr(scale), _ptr(shift),
            out.data_ptr(), ybs, b, cin, cout, split, h, w, w1[0], w1[1], w2[0], w2[1], _flags(relu), LEA_F32,
            probe=record)
    return out


def conv2d_bnrelu_pair(x: torch.Tensor, packed: torch.Tensor, c1: int, cout: int,
                       scale: torch.Tensor | None, shift: torch.Tensor | None, relu: bool,
                       out1: torch.Tensor, out2: torch.Tensor,
                       residual: torch.Tensor | None = None) -> None:
    """Two ConvBR2d 3x3/s1/p1 of x [B, cin, 1, H, W] in one launch (lea_conv2d_bnrelu_pair):
    ``packed`` holds both weight stacks along cout; couts [0, c1) go to ``out1`` (plus the
    ``residual``, the cell's skip term), [c1, cout) to ``out2`` ([B, cout - c1, 1, H, W] views,
    e.g. two non-adjacent slots of a cell's cat buffer)."""
    _require_cuda(x, packed, scale, shift, out1, out2, residual)
    b, cin, d, h, w = x.shape
    if d != 1:
        raise ValueError("conv2d_bnrelu_pair takes [B, C, 1, H, W] views")
    xbs = _check_volume_view(x, "x")
    if tuple(out1.shape) != (b, c1, 1, h, w) or tuple(out2.shape) != (b, cout - c1, 1, h, w):
        raise ValueError(f"conv2d_bnrelu_pair: outputs {tuple(out1.shape)} / {tuple(out2.shape)}")
    y1bs, y2bs = _check_volume_view(out1, "out1"), _check_volume_view(out2, "out2")
    rbs = 0
    if residual is not None:
        if tuple(residual.shape) != tuple(out1.shape):
            raise ValueError(f"conv2d_bnrelu_pair: residual {tuple(residual.shape)}")
        rbs = _check_volume_view(residual, "residual")
    _launch("lea_conv2d_bnrelu_pair", x.data_ptr(), xbs, packed.data_ptr(), _ptr(scale), _ptr(shift),
            _ptr(residual), rbs, out1.data_ptr(), y1bs, out2.data_ptr(), y2bs, b, cin, cout, c1, h, w,
            _flags(relu, residual is not None),
            probe=lambda: _op_record(
                conv2d_kernel_name(b, cout, h, w, cin), 2.0 * b * h * w * cout * cin * 9,
                4.0 * b * h * w * (cin + cout + (c1 if residual is not None else 0)) + 36.0 * cout * cin))


def feature_stem(x: torch.Tensor, w0: torch.Tensor, scale0, shift0, w1: torch.Tensor, scale1, shift1,
                 c8: bool = False, x2: torch.Tensor | None = None) -> torch.Tensor:
    """new_model_2d.py:93-94 fused (ConvBR 3x3 s1 then ConvBR 3x3 s3, BN + ReLU each):
    x [B, cin, H, W] f32 -> [B, c1, 1, Ho, Wo] f32, or c8 [B, c1/8, 1, Ho, Wo, 8] bf16.
    With ``x2`` (same shape) the output stacks both, [x; x2] along the batch, without
    a concatenated copy of the images: one launch per source, or for one image each a
    single launch whose batch stride is the distance between the two images."""
    _require_cuda(x, x2, scale0, shift0, scale1, shift1)
    w0, w1 = w0.detach().contiguous(), w1.detach().contiguous()
    _require_cuda(w0, w1)
    x = x.contiguous()
    srcs = [x]
    if x2 is not None:
        if tuple(x2.shape) != tuple(x.shape):
            raise ValueError(f"feature_stem: x2 {tuple(x2.shape)} differs from x {tuple(x.shape)}")
        x2 = x2.contiguous()  # both branches below read this tensor (pointer difference too)
        srcs.append(x2)
    b, cin, hi, wi = x.shape
    c0, c1 = w0.shape[0], w1.shape[0]
    if tuple(w0.shape) != (c0, cin, 3, 3) or tuple(w1.shape) != (c1, c0, 3, 3):
        raise ValueError(f"feature_stem: weights {tuple(w0.shape)} / {tuple(w1.shape)} do not chain")
    ho, wo = (hi - 1) // 3 + 1, (wi - 1) // 3 + 1
    nb = b * len(srcs)
    if c8:
        out = torch.empty((nb, c1 // 8, 1, ho, wo, 8), device=x.device, dtype=torch.bfloat16)
    else:
        out = torch.empty((nb, c1, 1, ho, wo), device=x.device, dtype=torch.float32)
    if len(srcs) == 2 and b == 1:
        # one image per source: one launch whose batch stride is the distance between them
        srcs, b, xbs = [x], 2, (x2.data_ptr() - x.data_ptr()) // x.element_size()
    else:
        xbs = x.stride(0)
    with _timed(lambda: _op_record(
            "feature_stem_kernel", 2.0 * nb * ho * wo * (9 * 9 * cin * c0 + 9 * c0 * c1),
            4.0 * nb * cin * hi * wi + out.numel() * out.element_size(), 0.0)):
        for i, src in enumerate(srcs):
            _launch("lea_feature_stem_bnrelu", src.data_ptr(), xbs, w0.data_ptr(), _ptr(scale0), _ptr(shift0),
                    w1.data_ptr(), _ptr(scale1), _ptr(shift1), out[i * b:].data_ptr(), out.stride(0), b, cin, c0,
                    c1, hi, wi, LEA_BF16 if c8 else LEA_F32)
    return out


def conv2d_s3_bnrelu(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor | None,
                     shift: torch.Tensor | None, relu: bool = True) -> torch.Tensor:
    """ConvBR2d 3x3, stride 3, pad 1 (new_model_2d.py:94) on x [B, cin, 1, H, W]."""
    _require_cuda(x, w, scale, shift)
    b, cin, d, hi, wi = x.shape
    if d != 1:
        raise ValueError("conv2d_s3_bnrelu takes [B, C, 1, H, W] views")
    w = w.detach().contiguous()
    cout = w.shape[0]
    if tuple(w.shape) != (cout, cin, 3, 3):
        raise ValueError(f"weight {tuple(w.shape)} does not match cin={cin}")
    xbs = _check_volume_view(x, "x")
    out = torch.empty((b, cout, 1, (hi - 1) // 3 + 1, (wi - 1) // 3 + 1), device=x.device,
                      dtype=x.dtype)
    _launch("lea_conv2d_s3_bnrelu", x.data_ptr(), xbs, w.data_ptr(), _ptr(scale), _ptr(shift), out.data_ptr(),
            out.stride(0), b, cin, cout, hi, wi, _flags(relu), LEA_F32,
            probe=lambda: _op_record("conv2d_s3_kernel", 2.0 * out.numel() * cin * 9,
                                     4.0 * (x.numel() + out.numel()), 0.0))
    return out


def resample_trilinear(x: torch.Tensor, size, align_corners: bool = True,
                       out: torch.Tensor | None = None, scale: torch.Tensor | None = None,
                       shift: torch.Tensor | None = None, relu: bool = False) -> torch.Tensor:
    """F.interpolate(x, size, mode='trilinear', align_corners=...) for NCDHW, with
    an optional per-channel ``relu(scale * . + shift)`` epilogue; ``out`` may be a
    channel slice of a larger tensor."""
    _require_cuda(x, out, scale, shift)
    b, c, di, hi, wi = x.shape
    do, ho, wo = (int(s) for s in size)
    xbs = _check_volume_view(x, "x")
    out, ybs = _out_view(out, (b, c, do, ho, wo), x.device)
    _launch("lea_resample3d_trilinear", x.data_ptr(), xbs, out.data_ptr(), ybs, b, c, di, hi, wi, do, ho, wo,
            1 if align_corners else 0, _ptr(scale), _ptr(shift), _flags(relu), LEA_F32,
            probe=lambda: _op_record("resample3d_f32", 0.0, 4.0 * b * c * (di * hi * wi + do * ho * wo)))
    return out


def resample_down2_shape_supported(in_size, size) -> bool:
    """lea_resample3d_down2_supported for f32: resampling ``in_size`` -> ``size`` (even D and H,
    W % 4 == 0, no down-sampling along D) with the half-size side output."""
    return bool(_lib.load().lea_resample3d_down2_supported(*(int(n) for n in in_size), *(int(n) for n in size),
                                                          LEA_F32))


def resample_down2_supported(x: torch.Tensor, size) -> bool:
    """Whether resample_trilinear_down2 takes x -> ``size``: an f32 NCDHW device tensor and a shape
    resample_down2_shape_supported accepts."""
    return _f32_volume(x, aligned=False) and resample_down2_shape_supported(x.shape[2:], size)


def resample_trilinear_down2(x: torch.Tensor, size, out: torch.Tensor | None = None,
                             down: torch.Tensor | None = None, scale: torch.Tensor | None = None,
                             shift: torch.Tensor | None = None, relu: bool = False):
    """(y, y2): y = resample_trilinear(x, size, True, out, scale, shift, relu) and y2 =
    resample_trilinear(y, size / 2), both bit for bit, as one launch that never reads y back;
    ``out`` / ``down`` may be channel slices of larger tensors."""
    _require_cuda(x, out, down, scale, shift)
    b, c, di, hi, wi = x.shape
    do, ho, wo = (int(n) for n in size)
    xbs = _check_volume_view(x, "x")
    out, ybs = _out_view(out, (b, c, do, ho, wo), x.device)
    down, dbs = _out_view(down, (b, c, do // 2, ho // 2, wo // 2), x.device, name="down")
    _launch("lea_resample3d_trilinear_down2", x.data_ptr(), xbs, out.data_ptr(), ybs, down.data_ptr(), dbs, b, c,
            di, hi, wi, do, ho, wo, _ptr(scale), _ptr(shift), _flags(relu), LEA_F32,
            probe=lambda: _op_record("resample3d_sep_down2_f32", 0.0,
                                     4.0 * (x.numel() + out.numel() + down.numel())))
    return out, down


def _tapsum(q, qbs, cout, in_size, size, scale, shift, relu, dtype, probe):
    """lea_tapsum_upsample of q (either layout, ``dtype`` LEA_F32 / LEA_BF16) -> f32 NCDHW."""
    b, (di, hi, wi) = q.shape[0], in_size
    do, ho, wo = (int(s) for s in size)
    out = torch.empty((b, cout, do, ho, wo), device=q.device, dtype=torch.float32)
    ws = torch.empty(_lib.load().lea_tapsum_workspace_bytes(b, cout, hi, wi, do) // 4, device=q.device,
                     dtype=torch.float32)
    _launch("lea_tapsum_upsample", q.data_ptr(), qbs, out.data_ptr(), out.stride(0), b, cout, di, hi, wi, do, ho,
            wo, _ptr(scale), _ptr(shift), _flags(relu), ws.data_ptr(), dtype, probe=lambda: probe(out))
    return out


def tapsum_upsample(q: torch.Tensor, cout: int, size, scale: torch.Tensor | None = None,
                    shift: torch.Tensor | None = None, relu: bool = False) -> torch.Tensor:
    """conv3x3x3(upsample(y)) from q = per-tap partial sums of y (27*cout channels at
    the low resolution): see include/leastereo_hip.h lea_tapsum_upsample."""
    _require_cuda(q, scale, shift)
    b, c27, di, hi, wi = q.shape
    if c27 != 27 * cout:
        raise ValueError(f"q has {c27} channels, expected 27*{cout}")
    return _tapsum(q, _check_volume_view(q, "q"), cout, (di, hi, wi), size, scale, shift, relu, LEA_F32,
                   lambda out: _op_record("tapsum_f32", 0.0, 4.0 * (b * c27 * di * hi * wi + out.numel())))


def disparity_regression(cost: torch.Tensor, maxdisp: int, fast_exp: bool = False) -> torch.Tensor:
    """Disp + DisparityRegression (build_model_2d.py:52-57, 33-42): [B,1,D3,H3,W3] -> [B,3H3,3W3].
    ``fast_exp``: hardware exp (the bf16 path)."""
    cost, b, d3, h3, w3 = _head_cost(cost)
    disp = torch.empty((b, 3 * h3, 3 * w3), device=cost.device, dtype=torch.float32)
    _launch("lea_disparity_regression", cost.data_ptr(), disp.data_ptr(), b, d3, h3, w3, maxdisp,
            LEA_BF16 if fast_exp else LEA_F32,
            probe=lambda: _op_record("disparity_regression", 0.0, 4.0 * (cost.numel() + disp.numel())))
    return disp


class DisparityStats(collections.namedtuple("DisparityStats", "disp entropy peak disp_local")):
    """What ``disparity_regression_stats`` returns: the disparity and, per pixel, what the
    softmin distribution over ``maxdisp`` says about it (``None`` where not asked for).
    All [B, 3H3, 3W3] float32, none differentiable.
      entropy     -sum p ln p, nats, [0, ln maxdisp]
      peak        the probability mass within ``radius`` of the winner, (0, 1]
      disp_local  the soft-argmin of that window
    ``maxdisp`` (an attribute, not a field) is what ``confidence`` normalises by."""

    def __new__(cls, disp, entropy=None, peak=None, disp_local=None, maxdisp=None):
        self = super().__new__(cls, disp, entropy, peak, disp_local)
        self.maxdisp = maxdisp
        return self

    @property
    def confidence(self) -> torch.Tensor:
        """``1 - entropy / ln(maxdisp)``: 0 = a flat distribution, 1 = a single disparity."""
        if self.entropy is None or not self.maxdisp:
            raise ValueError("confidence needs the entropy output (entropy=True) and maxdisp")
        return 1.0 - self.entropy / math.log(self.maxdisp)


def disparity_regression_stats(cost: torch.Tensor, maxdisp: int, radius: int = 4, fast_exp: bool = False,
                               entropy: bool = True, peak: bool = True, local: bool = True) -> DisparityStats:
    """``disparity_regression`` that also returns the per-pixel confidence measures of
    ``lea_disparity_regression_stats`` (include/leastereo_hip.h) from the same launch:
    [B,1,D3,H3,W3] -> DisparityStats of [B,3H3,3W3].  ``disp`` is ``disparity_regression``'s
    bit for bit at the configured depths.  ``maxdisp`` must be 3 * D3."""
    cost, b, d3, h3, w3 = _head_cost(cost)
    if not (entropy or peak or local):
        raise ValueError("disparity_regression_stats: ask for at least one of entropy, peak, local "
                         "(disparity_regression gives the disparity alone)")
    # one allocation per output: a hole (an output not asked for) is a null pointer
    outs = [torch.empty((b, 3 * h3, 3 * w3), device=cost.device, dtype=torch.float32) if want else None
            for want in (True, entropy, peak, local)]
    _launch("lea_disparity_regression_stats", cost.data_ptr(), *map(_ptr, outs), b, d3, h3, w3, maxdisp, radius,
            LEA_BF16 if fast_exp else LEA_F32,
            probe=lambda: _op_record("disparity_regression_stats", 0.0,
                                     4.0 * (cost.numel() + sum(o.numel() for o in outs if o is not None))))
    return DisparityStats(*outs, maxdisp)


LR_CONSISTENT, LR_INCONSISTENT, LR_OUT_OF_VIEW = 0, 1, 2
LR_SPECKLE = 3  # written by ``speckle_filter`` into the same state map

DisparityLR = collections.namedtuple("DisparityLR", "disp disp_right state disp_filled")
DisparityLR.__doc__ = """What ``LEAStereo.forward_lr`` / ``lr_check`` return (``None`` where not asked for):
  disp         the left-view disparity, [B, H, W] float32
  disp_right   the right-view disparity read off the same cost (``disparity_regression_right``)
  state        uint8: LR_CONSISTENT, LR_INCONSISTENT (occluded or mismatched), LR_OUT_OF_VIEW
  disp_filled  ``disp`` where consistent, elsewhere the smaller of the nearest consistent
               disparities to the left and right on the row
None differentiable."""


def disparity_regression_right(cost: torch.Tensor, maxdisp: int, fast_exp: bool = False) -> torch.Tensor:
    """The right view's disparity from the left view's matching cost
    (``lea_disparity_regression_right``, include/leastereo_hip.h): the up-sampled cost read
    along its diagonals, right pixel xr at disparity od being left pixel xr + od, soft-argmin
    over the candidates in view.  [B,1,D3,H3,W3] -> [B,3H3,3W3]; ``maxdisp`` must be 3 * D3."""
    cost, b, d3, h3, w3 = _head_cost(cost)
    out = torch.empty((b, 3 * h3, 3 * w3), device=cost.device, dtype=torch.float32)
    _launch("lea_disparity_regression_right", cost.data_ptr(), out.data_ptr(), b, d3, h3, w3, maxdisp,
            LEA_BF16 if fast_exp else LEA_F32,
            probe=lambda: _op_record("disparity_regression_right", 0.0, 4.0 * (cost.numel() + out.numel())))
    return out


def lr_check(disp_left: torch.Tensor, disp_right: torch.Tensor, threshold: float = 1.0, want_state: bool = True,
             want_filled: bool = True) -> DisparityLR:
    """The left-right consistency check and scanline fill of ``lea_disparity_lr_check``
    (include/leastereo_hip.h) in one launch: two [B, H, W] float32 disparities ->
    ``DisparityLR(disp_left, disp_right, state, disp_filled)``."""
    _require_cuda(disp_left, disp_right)
    if disp_left.dim() != 3 or disp_left.shape != disp_right.shape:
        raise ValueError("disp_left and disp_right must be [B, H, W] of one shape")
    if not (want_state or want_filled):
        raise ValueError("lr_check: ask for at least one of state, filled")
    dl, dr = disp_left.contiguous(), disp_right.contiguous()
    b, h, w = dl.shape
    state = torch.empty((b, h, w), device=dl.device, dtype=torch.uint8) if want_state else None
    filled = torch.empty((b, h, w), device=dl.device, dtype=torch.float32) if want_filled else None
    _launch("lea_disparity_lr_check", dl.data_ptr(), dr.data_ptr(), _ptr(state), _ptr(filled), b, h, w,
            float(threshold),
            probe=lambda: _op_record("disparity_lr_check", 0.0, dl.numel() * (
                8.0 + (1.0 if want_state else 0.0) + (16.0 if want_filled else 0.0))))
    return DisparityLR(disp_left, disp_right, state, filled)


# ---- edge-aware training loss (csrc/median.hip, csrc/edge_loss.hip) ----

def _plane_view(t: torch.Tensor, name: str):
    """[B, H, W] float32 whose (H, W) block is contiguous per batch (a copy if it is not);
    returns the tensor and its batch stride in elements."""
    b, h, w = t.shape
    if t.stride()[1:] != (w, 1) or (b > 1 and t.stride(0) < h * w):
        t = t.contiguous()
    return t, (t.stride(0) if b > 1 else h * w)


def median_blur5(x: torch.Tensor, iterations: int = 1) -> torch.Tensor:
    """Exact 5x5 median with a replicated border (``lea_median5x5_f32``: OpenCV's
    ``medianBlur(x, 5)``), applied ``iterations`` (1 or 2) times in one launch.
    [B, H, W] or [H, W] float32 on the ROCm device, NaN-free; returns the same shape."""
    _require_cuda(x)
    if x.dim() not in (2, 3):
        raise ValueError(f"median_blur5: [B, H, W] or [H, W] expected, got {tuple(x.shape)}")
    if iterations not in (1, 2):
        raise ValueError("median_blur5: iterations must be 1 or 2")
    x3 = x.unsqueeze(0) if x.dim() == 2 else x
    x3, xbs = _plane_view(x3, "x")
    b, h, w = x3.shape
    y = torch.empty((b, h, w), device=x.device, dtype=torch.float32)
    _launch("lea_median5x5_f32", x3.data_ptr(), xbs, y.data_ptr(), h * w, b, h, w, int(iterations),
            probe=lambda: _op_record("median5x5", 0.0, 8.0 * y.numel()))
    return y.squeeze(0) if x.dim() == 2 else y


EDGE_LOSS_FIELDS = ("n_valid", "sum_smooth_l1", "sum_abs", "sum_edge")


def _edge_maps(pred, target, tsmooth):
    _require_cuda(pred, target, tsmooth)
    if pred.dim() != 3 or pred.shape != target.shape or pred.shape != tsmooth.shape:
        raise ValueError("pred, target and tsmooth must be [B, H, W] of one shape")
    if pred.shape[1] < 3 or pred.shape[2] < 3:
        raise ValueError("the edge term needs H >= 3 and W >= 3")
    return _plane_view(pred, "pred"), _plane_view(target, "target"), _plane_view(tsmooth, "tsmooth")


def edge_loss_sums(pred: torch.Tensor, target: torch.Tensor, tsmooth: torch.Tensor, maxdisp: float) -> torch.Tensor:
    """The four sums of ``lea_edge_loss_f32`` (include/leastereo_hip.h), float64 [4] on the
    device in the order of ``EDGE_LOSS_FIELDS``; nothing is read back."""
    (p, pbs), (t, tbs), (s, sbs) = _edge_maps(pred, target, tsmooth)
    b, h, w = p.shape
    ws = torch.empty(_lib.load().lea_edge_loss_workspace_bytes(b, h, w) // 8, device=p.device, dtype=torch.float64)
    sums = torch.empty(4, device=p.device, dtype=torch.float64)
    _launch("lea_edge_loss_f32", p.data_ptr(), pbs, t.data_ptr(), tbs, s.data_ptr(), sbs, b, h, w, float(maxdisp),
            sums.data_ptr(), ws.data_ptr(), probe=lambda: _op_record("edge_loss", 0.0, 12.0 * p.numel()))
    return sums


def edge_loss_grad(pred: torch.Tensor, target: torch.Tensor, tsmooth: torch.Tensor, maxdisp: float,
                   sums: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """``lea_edge_loss_grad_f32``: the gradient with respect to ``pred`` of
    ``scales[0] * direct + scales[1] * edge``; ``sums`` is what ``edge_loss_sums`` returned
    for the same maps, ``scales`` two float32 on the device."""
    (p, pbs), (t, tbs), (s, sbs) = _edge_maps(pred, target, tsmooth)
    _sums_scales(sums, scales, "edge_loss_sums", "g_direct, g_edge")
    b, h, w = p.shape
    dpred = torch.empty((b, h, w), device=p.device, dtype=torch.float32)
    _launch("lea_edge_loss_grad_f32", p.data_ptr(), pbs, t.data_ptr(), tbs, s.data_ptr(), sbs, sums.data_ptr(),
            scales.data_ptr(), dpred.data_ptr(), h * w, b, h, w, float(maxdisp),
            probe=lambda: _op_record("edge_loss_grad", 0.0, 16.0 * p.numel()))
    return dpred


# ---- photometric consistency (csrc/photometric.hip) ----

PHOTOMETRIC_FIELDS = ("n_view", "sum_l1", "n_window", "sum_dssim")
PHOTO_C1, PHOTO_C2 = 0.01 ** 2, 0.03 ** 2


def _image_view(t: torch.Tensor):
    """[B, C, H, W] float32 whose (C, H, W) block is contiguous per batch (a copy if it is
    not); returns the tensor and its batch stride in elements."""
    b, c, h, w = t.shape
    if t.stride()[1:] != (h * w, w, 1) or (b > 1 and t.stride(0) < c * h * w):
        t = t.contiguous()
    return t, (t.stride(0) if b > 1 else c * h * w)


def _photo_maps(left, right, disp, exclude):
    _require_cuda(left, right, disp)
    if left.dim() != 4 or left.shape != right.shape:
        raise ValueError("left and right must be [B, C, H, W] of one shape")
    b, c, h, w = left.shape
    if not 1 <= c <= 4:
        raise ValueError(f"photometric: 1 <= C <= 4 channels, got {c}")
    if h < 3 or w < 3:
        raise ValueError("photometric: H >= 3 and W >= 3 are needed")
    if tuple(disp.shape) != (b, h, w):
        raise ValueError(f"disp must be [B, H, W] = {(b, h, w)}, got {tuple(disp.shape)}")
    e = _exclude_u8(exclude, (b, h, w))
    return (_image_view(left), _image_view(right), _plane_view(disp, "disp"),
            (None, 0) if e is None else _plane_view(e, "exclude"))


def photometric_sums(left: torch.Tensor, right: torch.Tensor, disp: torch.Tensor, exclude: torch.Tensor = None,
                     alpha: float = 0.85, c1: float = PHOTO_C1, c2: float = PHOTO_C2, want_warped: bool = False,
                     want_err: bool = False):
    """The four sums of ``lea_photometric_f32`` (include/leastereo_hip.h), float64 [4] on the
    device in the order of ``PHOTOMETRIC_FIELDS``; nothing is read back.  With ``want_warped``
    or ``want_err`` returns ``(sums, warped, err)``, the map not asked for being None."""
    (l, lbs), (r, rbs), (d, dbs), (e, ebs) = _photo_maps(left, right, disp, exclude)
    b, c, h, w = l.shape
    ws = torch.empty(_lib.load().lea_photometric_workspace_bytes(b, h, w) // 8, device=l.device,
                     dtype=torch.float64)
    sums = torch.empty(4, device=l.device, dtype=torch.float64)
    warped = torch.empty((b, c, h, w), device=l.device, dtype=torch.float32) if want_warped else None
    err = torch.empty((b, h, w), device=l.device, dtype=torch.float32) if want_err else None
    _launch("lea_photometric_f32", l.data_ptr(), lbs, r.data_ptr(), rbs, d.data_ptr(), dbs, _ptr(e), ebs, b, c, h,
            w, float(alpha), float(c1), float(c2), sums.data_ptr(), ws.data_ptr(), _ptr(warped), _ptr(err),
            probe=lambda: _op_record("photometric", 0.0, 4.0 * (l.numel() + r.numel() + d.numel())))
    return (sums, warped, err) if (want_warped or want_err) else sums


def photometric_grad(left: torch.Tensor, right: torch.Tensor, disp: torch.Tensor, exclude: torch.Tensor = None,
                     c1: float = PHOTO_C1, c2: float = PHOTO_C2, *, sums: torch.Tensor,
                     scales: torch.Tensor) -> torch.Tensor:
    """``lea_photometric_grad_f32``: the gradient with respect to ``disp`` of
    ``scales[0] * l1 + scales[1] * dssim`` (the two means); ``sums`` is what
    ``photometric_sums`` returned for the same inputs, ``scales`` two float32 on the device."""
    (l, lbs), (r, rbs), (d, dbs), (e, ebs) = _photo_maps(left, right, disp, exclude)
    _sums_scales(sums, scales, "photometric_sums", "g_l1, g_dssim")
    b, c, h, w = l.shape
    ddisp = torch.empty((b, h, w), device=l.device, dtype=torch.float32)
    _launch("lea_photometric_grad_f32", l.data_ptr(), lbs, r.data_ptr(), rbs, d.data_ptr(), dbs, _ptr(e), ebs, b,
            c, h, w, float(c1), float(c2), sums.data_ptr(), scales.data_ptr(), ddisp.data_ptr(), h * w,
            probe=lambda: _op_record("photometric_grad", 0.0, 4.0 * (l.numel() + r.numel() + 2 * d.numel())))
    return ddisp


# ---- confidence-weighted edge-preserving refinement (csrc/refine.hip) ----

REFINE_LAMBDA, REFINE_SIGMA, REFINE_ITERATIONS = 8000.0, 0.05, 3

DisparityRefined = collections.namedtuple("DisparityRefined", "disp disp_refined support peak disp_right state")
DisparityRefined.__doc__ = """What ``LEAStereo.forward_refined`` returns, all [B, H, W]:
  disp          the left-view disparity of ``forward``, bit for bit
  disp_refined  ``fgs_refine`` of it: guide the left image, conf ``peak``, exclude ``state``
  support       how much confident evidence reached each pixel (the smoothed confidence)
  peak          the peak mass of ``forward_with_confidence``
  disp_right    the right view's disparity of ``forward_lr``
  state         uint8, the left-right check's state of ``forward_lr``
None differentiable."""


def fgs_refine(guide: torch.Tensor, disp: torch.Tensor, conf: torch.Tensor = None, exclude: torch.Tensor = None,
               lam: float = REFINE_LAMBDA, sigma: float = REFINE_SIGMA, iterations: int = REFINE_ITERATIONS,
               return_support: bool = False):
    """``lea_disparity_refine_f32`` (include/leastereo_hip.h): the confidence-weighted,
    image-guided weighted-least-squares smoothing of a disparity map by the fast global
    smoother.  ``guide`` [B, C, H, W] float32 with 1 <= C <= 4 (a channel slice of a larger
    tensor goes as a view), ``disp`` [B, H, W] float32, ``conf`` [B, H, W] float32 or None
    (= 1), ``exclude`` [B, H, W] uint8 or bool or None (non-zero = no evidence;
    ``DisparityLR.state`` goes as it is).  ``sigma`` is in the guide's units.  Returns the
    refined disparity [B, H, W], with ``return_support`` (refined, support).  2 + 4 *
    ``iterations`` launches on the current stream; nothing is read back."""
    _require_cuda(guide, disp, conf)
    if guide.dim() != 4 or not 1 <= guide.shape[1] <= 4:
        raise ValueError(f"fgs_refine: guide must be [B, C, H, W] with 1 <= C <= 4, got {tuple(guide.shape)}")
    b, c, h, w = guide.shape
    if tuple(disp.shape) != (b, h, w):
        raise ValueError(f"disp must be [B, H, W] = {(b, h, w)}, got {tuple(disp.shape)}")
    if conf is not None and tuple(conf.shape) != (b, h, w):
        raise ValueError(f"conf must be [B, H, W] = {(b, h, w)}, got {tuple(conf.shape)}")
    e = _contiguous(_exclude_u8(exclude, (b, h, w)))
    if not (lam > 0 and math.isfinite(lam) and sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"fgs_refine: lam {lam} and sigma {sigma} must be finite numbers > 0")
    if not 1 <= int(iterations) <= 8 or int(iterations) != iterations:
        raise ValueError(f"fgs_refine: iterations {iterations} (1..8)")
    g, gbs = _image_view(guide)
    d = disp.contiguous()
    cf = _contiguous(conf)
    ws = torch.empty(_lib.load().lea_disparity_refine_workspace_bytes(b, h, w) // 4, device=d.device,
                     dtype=torch.float32)
    refined = torch.empty((b, h, w), device=d.device, dtype=torch.float32)
    support = torch.empty_like(refined) if return_support else None
    _launch("lea_disparity_refine_f32", g.data_ptr(), gbs, d.data_ptr(), _ptr(cf), _ptr(e), b, c, h, w, float(lam),
            float(sigma), int(iterations), ws.data_ptr(), refined.data_ptr(), _ptr(support),
            probe=lambda: _op_record("disparity_refine", 0.0, 4.0 * d.numel() * (c + 3 + 22 * iterations)))
    return (refined, support) if return_support else refined


# ---- speckle filter: connected components of the disparity (csrc/speckle.hip) ----

SPECKLE_MAX_SIZE, SPECKLE_MAX_DIFF = 200, 1.0

DisparitySpeckle = collections.namedtuple("DisparitySpeckle", "disp state size labels filtered")
DisparitySpeckle.__doc__ = """What ``speckle_filter`` returns, all [B, H, W] (``None`` where not asked for):
  disp      the input, as it was given
  state     uint8: ``exclude`` where that is non-zero, elsewhere ``LR_SPECKLE`` (3) on the removed pixels, else 0
  size      int32: the pixel count of the pixel's component, 0 for a wall
  labels    int32: the smallest linear index y * W + x of the pixel's component, -1 for a wall
  filtered  float32: ``fill`` where state != 0, ``disp`` bit for bit elsewhere
None differentiable."""


def _disparity_map(who, disp):
    """The [B, H, W] or [H, W] float32 device disparity of the post-processing calls; its shape."""
    if not isinstance(disp, torch.Tensor) or disp.dim() not in (2, 3):
        raise ValueError(f"{who}: disp must be [B, H, W] or [H, W], got "
                         f"{tuple(disp.shape) if isinstance(disp, torch.Tensor) else type(disp)}")
    _require_cuda(disp)
    return tuple(disp.shape)


def speckle_filter(disp: torch.Tensor, exclude: torch.Tensor = None, max_size: int = SPECKLE_MAX_SIZE,
                   max_diff: float = SPECKLE_MAX_DIFF, fill: float = 0.0, want_labels: bool = False,
                   want_size: bool = True, want_filtered: bool = True) -> DisparitySpeckle:
    """``lea_disparity_speckle_f32`` (include/leastereo_hip.h): the 4-connected components of a
    disparity map (two neighbours connected when |a - b| <= ``max_diff`` px; a non-finite or
    excluded pixel is a wall) and the removal of those of at most ``max_size`` pixels, OpenCV's
    ``filterSpeckles``.  ``disp`` [B, H, W] or [H, W] float32 on the device, ``exclude`` of the
    same shape, uint8 or bool, or None (``DisparityLR.state`` goes as it is, and its values come
    back in ``state``).  Returns ``DisparitySpeckle``; ``state`` is always computed.  The
    defaults (200 px, 1.0 px) are the middle of OpenCV's recommended 50-200 window and 1-2
    range and are **untuned**: there is no trained checkpoint and no real pair here to tune
    them on.  Four launches on the current stream; nothing is read back."""
    who = "speckle_filter"
    shape = _disparity_map(who, disp)
    e = _exclude_u8(exclude, shape, who)
    _number(who, "max_diff", max_diff, "a finite number >= 0", lo=0, finite=True)
    _number(who, "max_size", max_size, "an integer in 0 .. 2^31 - 1", lo=0, hi=2 ** 31 - 1, integer=True)
    _number(who, "fill", fill, "a number", bools=True)
    if 0 in shape:
        raise ValueError(f"speckle_filter: empty map {shape}")
    if shape[-2] * shape[-1] >= 2 ** 31:
        raise ValueError(f"speckle_filter: H * W = {shape[-2] * shape[-1]} is not below 2^31")
    d = disp.contiguous()
    e = _contiguous(e)
    b = shape[0] if len(shape) == 3 else 1
    h, w = shape[-2:]
    ws = torch.empty(_lib.load().lea_disparity_speckle_workspace_bytes(b, h, w) // 4, device=d.device,
                     dtype=torch.int32)
    state = torch.empty(shape, device=d.device, dtype=torch.uint8)
    size = torch.empty(shape, device=d.device, dtype=torch.int32) if want_size else None
    labels = torch.empty(shape, device=d.device, dtype=torch.int32) if want_labels else None
    filtered = torch.empty(shape, device=d.device, dtype=torch.float32) if want_filtered else None
    _launch("lea_disparity_speckle_f32", d.data_ptr(), _ptr(e), b, h, w, float(max_diff), int(max_size),
            float(fill), ws.data_ptr(), _ptr(labels), _ptr(size), state.data_ptr(), _ptr(filtered),
            probe=lambda: _op_record("disparity_speckle", 0.0, d.numel() * (
                30.0 + (4.0 if want_size else 0.0) + (4.0 if want_labels else 0.0) +
                (8.0 if want_filtered else 0.0))))
    return DisparitySpeckle(disp, state, size, labels, filtered)


# ---- point cloud: reprojection, ordered compaction, normals (csrc/pointcloud.hip) ----

HostPointCloud = collections.namedtuple("HostPointCloud", "count xyz rgb index normals")
HostPointCloud.__doc__ = """What ``PointCloud.to_host`` returns: ``count`` (int, the valid pixels of the item, which may
exceed the rows) and the first min(count, capacity) rows of each compact array as numpy arrays (``None`` where the
call did not make one)."""


class PointCloud(collections.namedtuple("PointCloud", "points valid count xyz rgb index normals")):
    """What ``reproject`` returns, on the device (``None`` where not asked for):
      points   float32 [B, H, W, 3]: the organised cloud, NaN in all three where the pixel is not valid
      valid    uint8 [B, H, W]: 1 / 0
      count    int32 [B]: the number of valid pixels, also where it exceeds the capacity
      xyz      float32 [B, capacity, 3]: the valid points in row-major pixel order
      rgb      uint8 [B, capacity, 3]: their colours
      index    int32 [B, capacity]: their y * W + x
      normals  float32 [B, capacity, 3]: their normals, towards the camera; (0, 0, 0) where there is none
    The leading B is absent where ``disp`` came as [H, W].  Rows at and beyond min(count, capacity) are
    uninitialised memory: ``to_host`` cuts them off."""
    __slots__ = ()

    def to_host(self, b: int = 0) -> HostPointCloud:
        """The one place that synchronises: reads ``count[b]`` and copies the first min(count, capacity) rows of
        each compact array of item ``b`` to numpy."""
        if self.count is None:
            raise ValueError("PointCloud.to_host: the call made no compact output (want_compact=False)")
        batched = self.count.dim() == 1
        if not batched and b != 0:
            raise IndexError(f"PointCloud.to_host: item {b} of an unbatched cloud")
        n = int(self.count[b] if batched else self.count)
        rows = None
        out = []
        for t in (self.xyz, self.rgb, self.index, self.normals):
            if t is None:
                out.append(None)
                continue
            t = t[b] if batched else t
            rows = min(n, t.shape[0])
            out.append(t[:rows].cpu().numpy())
        return HostPointCloud(n, *out)


def _as_q(Q, b: int, device) -> torch.Tensor:
    """Q as a float32 tensor on the device, [4, 4] or [b, 4, 4]; one that is that already is used in
    place (a captured call then replays with what it holds at the time)."""
    shape = tuple(Q.shape) if isinstance(Q, torch.Tensor) else np.shape(Q)
    if shape not in ((4, 4), (b, 4, 4)):
        raise ValueError(f"reproject: Q must be [4, 4] or [{b}, 4, 4], got {shape}")
    return _as_f32(Q, device, "reproject: Q must be a floating-point matrix")


def reproject(disp: torch.Tensor, Q, image: torch.Tensor = None, exclude: torch.Tensor = None,
              min_disp: float = 0.0, max_disp: float = float("inf"), normals: bool = False,
              normal_max_diff: float = 1.0, capacity: int = None, want_points: bool = False,
              want_valid: bool = False, want_compact: bool = True) -> PointCloud:
    """``lea_disparity_pointcloud_f32`` (include/leastereo_hip.h): the points
    P = (h0, h1, h2) / h3, h = Q (x, y, d, 1), of the pixels of a disparity map that are valid
    (``exclude`` 0, d finite, ``min_disp`` < d <= ``max_disp``, P finite), organised
    (``want_points``, ``want_valid``) and compacted in row-major pixel order (``want_compact``:
    count, xyz, index; rgb with ``image``; ``normals=True`` for the normals, whose neighbours
    must lie within ``normal_max_diff`` px of disparity).  ``disp`` [B, H, W] or [H, W] float32
    on the device; ``Q`` a 4 x 4 or [B, 4, 4] array or tensor (``pointcloud.q_matrix``), a
    float32 device tensor is read in place at every launch and replay; ``image`` uint8
    [B, H, W, 3|4] or [H, W, 3|4] on the device (what ``load_images`` decodes); ``exclude`` as
    for ``speckle_filter`` (``DisparityLR.state`` / ``DisparitySpeckle.state`` go as they are).
    ``capacity``: rows per item of the compact arrays, H * W by default; the first ``capacity``
    points are kept.  Up to three launches on the current stream; nothing is read back, the
    number of points stays on the device (``PointCloud.to_host``)."""
    who = "reproject"
    shape = _disparity_map(who, disp)
    if 0 in shape:
        raise ValueError(f"reproject: empty map {shape}")
    batched = len(shape) == 3
    b = shape[0] if batched else 1
    h, w = shape[-2:]
    if b * h * w > 2 ** 31 - 1:
        raise ValueError(f"reproject: B * H * W = {b * h * w} is above 2^31 - 1")
    e = _exclude_u8(exclude, shape, who)
    img = None
    if image is not None:
        if (not isinstance(image, torch.Tensor) or not image.is_cuda or image.dtype != torch.uint8
                or tuple(image.shape[:-1]) != shape or image.shape[-1] not in (3, 4)):
            raise ValueError(f"reproject: image must be a uint8 {shape + ('3|4',)} tensor on the device")
        img = image.contiguous()
    for name, v in (("min_disp", min_disp), ("max_disp", max_disp), ("normal_max_diff", normal_max_diff)):
        _number(who, name, v, "a number", lo=-math.inf)
    _number(who, "normal_max_diff", normal_max_diff, ">= 0", lo=0)
    if capacity is None:
        capacity = h * w
    _number(who, "capacity", capacity, "an integer in 1 .. 2^31 - 1", lo=1, hi=2 ** 31 - 1, integer=True)
    if normals and not want_compact:
        raise ValueError("reproject: the normals are a compact output (want_compact=True)")
    if not (want_points or want_valid or want_compact):
        raise ValueError("reproject: nothing asked for")
    d = disp.contiguous()
    e = _contiguous(e)
    q = _as_q(Q, b, d.device)
    dev = d.device
    ws = torch.empty(_lib.load().lea_disparity_pointcloud_workspace_bytes(b, h, w) // 4, device=dev,
                     dtype=torch.int32)
    lead = (b,) if batched else ()
    new = lambda want, tail, dtype: torch.empty(lead + tail, device=dev, dtype=dtype) if want else None  # noqa: E731
    points = new(want_points, (h, w, 3), torch.float32)
    valid = new(want_valid, (h, w), torch.uint8)
    count = new(want_compact, (), torch.int32)
    xyz = new(want_compact, (capacity, 3), torch.float32)
    rgb = new(want_compact and img is not None, (capacity, 3), torch.uint8)
    index = new(want_compact, (capacity,), torch.int32)
    nrm = new(want_compact and normals, (capacity, 3), torch.float32)
    _launch("lea_disparity_pointcloud_f32", d.data_ptr(), _ptr(e), _ptr(img), 0 if img is None else img.shape[-1],
            q.data_ptr(), 16 if q.dim() == 3 else 0, b, h, w, float(min_disp), float(max_disp),
            float(normal_max_diff), int(capacity), ws.data_ptr(), _ptr(points), _ptr(valid), _ptr(count), _ptr(xyz),
            _ptr(rgb), _ptr(index), _ptr(nrm),
            probe=lambda: _op_record("disparity_pointcloud", 0.0, d.numel() * (
                (8.0 if want_compact else 4.0) + (0.0 if e is None else 1.0) +
                (12.0 if want_points else 0.0) + (1.0 if want_valid else 0.0) +
                (16.0 if want_compact else 0.0) + (0.0 if rgb is None else 6.0) +
                (12.0 if nrm is not None else 0.0))))
    return PointCloud(points, valid, count, xyz, rgb, index, nrm)


# ---- rectification of a raw pair: calibration or maps to images (csrc/rectify.hip) ----

RectifiedPair = collections.namedtuple("RectifiedPair", "left right valid maps")
RectifiedPair.__doc__ = """What ``rectify_u8`` returns, on the device: ``left`` / ``right`` uint8 [B, Ho, Wo, ps],
``valid`` uint8 [B, 2, Ho, Wo] (view, 1 / 0) and ``maps`` float32 [B, 2, 2, Ho, Wo] (view, then x / y: the source
coordinates the launch used), ``None`` where not asked for.  The leading B is absent where the images came as
[H, W, ps]."""

RECT_CALIB_FLOATS = 24


def rectify_u8(left: torch.Tensor, right: torch.Tensor, calib=None, maps=None, size=None, fill: int = 0,
               want_valid: bool = True, want_maps: bool = False) -> RectifiedPair:
    """``lea_rectify_pair_u8`` (include/leastereo_hip.h): both raw views of a batch undistorted
    and rectified in one launch, bilinear, every channel.  ``left`` / ``right`` uint8
    [B, H, W, 3|4] or [H, W, 3|4] on the device, as decoded.  Exactly one of ``calib``
    (float32 [1|B, 2, 24], ``rectify.Rectification.calib()``; a float32 device tensor is read
    in place at every launch and replay) and ``maps`` (float32 [1|B, 2, 2, Ho, Wo]: any lens
    model, maps made elsewhere).  ``size`` (Ho, Wo): the output's size with ``calib`` (default:
    the input's); with ``maps`` it is theirs.  Pixels whose source lies outside the raw image
    are ``fill`` in every channel and 0 in ``valid``.  The outputs feed ``standardize_crop_u8``,
    ``standardize_tiles_u8``, ``forward_scene``, ``reproject(image=...)`` as they are."""
    for t in (left, right):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
            raise ValueError("rectify_u8: left and right must be uint8 tensors on the device")
    if left.shape != right.shape or left.dim() not in (3, 4) or left.shape[-1] not in (3, 4) or 0 in left.shape:
        raise ValueError(f"rectify_u8: left / right must both be [B, H, W, 3|4] or [H, W, 3|4], got "
                         f"{tuple(left.shape)} and {tuple(right.shape)}")
    batched = left.dim() == 4
    if not batched:
        left, right = left.unsqueeze(0), right.unsqueeze(0)
    left, right = left.contiguous(), right.contiguous()
    b, h, w, ps = left.shape
    if (calib is None) == (maps is None):
        raise ValueError("rectify_u8: exactly one of calib and maps must be given")
    _number("rectify_u8", "fill", fill, "an integer in 0 .. 255", lo=0, hi=255, integer=True)
    dev = left.device
    c = m = None
    if calib is not None:
        c = _as_f32(calib, dev, "rectify_u8: calib must be floating point")
        if c.dim() == 2:
            c = c.unsqueeze(0)
        if c.dim() != 3 or tuple(c.shape[1:]) != (2, RECT_CALIB_FLOATS) or c.shape[0] not in (1, b):
            raise ValueError(f"rectify_u8: calib must be [1|{b}, 2, {RECT_CALIB_FLOATS}], got {tuple(c.shape)}")
        ho, wo = (h, w) if size is None else (int(size[0]), int(size[1]))
    else:
        m = _as_f32(maps, dev, "rectify_u8: maps must be floating point")
        if m.dim() == 4:
            m = m.unsqueeze(0)
        if m.dim() != 5 or tuple(m.shape[1:3]) != (2, 2) or m.shape[0] not in (1, b) or 0 in m.shape:
            raise ValueError(f"rectify_u8: maps must be [1|{b}, 2, 2, Ho, Wo], got {tuple(m.shape)}")
        ho, wo = m.shape[-2:]
        if size is not None and (int(size[0]), int(size[1])) != (ho, wo):
            raise ValueError(f"rectify_u8: size {tuple(size)} contradicts the maps' {(ho, wo)}")
    if not (1 <= ho <= 65535 and 1 <= wo <= 65535):
        raise ValueError(f"rectify_u8: output size {(ho, wo)} outside 1 .. 65535")
    out_l = torch.empty((b, ho, wo, ps), device=dev, dtype=torch.uint8)
    out_r = torch.empty_like(out_l)
    valid = torch.empty((b, 2, ho, wo), device=dev, dtype=torch.uint8) if want_valid else None
    mo = torch.empty((b, 2, 2, ho, wo), device=dev, dtype=torch.float32) if want_maps else None
    n = 2.0 * b * ho * wo
    _launch("lea_rectify_pair_u8", left.data_ptr(), right.data_ptr(), ps, b, h, w, _ptr(c),
            0 if c is None else c.shape[0], _ptr(m), 0 if m is None else m.shape[0], ho, wo, int(fill),
            out_l.data_ptr(), out_r.data_ptr(), _ptr(valid), _ptr(mo),
            probe=lambda: _op_record("rectify_pair", 50.0 * n, n * (
                2.0 * ps + (1.0 if want_valid else 0.0) + (8.0 if want_maps else 0.0) +
                (8.0 if m is not None else 0.0))))
    outs = (out_l, out_r, valid, mo)
    if not batched:
        outs = tuple(None if t is None else t[0] for t in outs)
    return RectifiedPair(*outs)


# ---- view synthesis: forward warp with occlusion and fill (csrc/forward_warp.hip) ----

FORWARD_WARP_MAX_W = 4096  # LEA_FORWARD_WARP_MAX_W


class WarpedView(collections.namedtuple("WarpedView", "image zview state source")):
    """What ``forward_warp`` returns, on the device (``None`` where not asked for):
      image   float32 [B, C, H, W]: the view; holes filled from the background, or ``fill_value``
      zview   float32 [B, H, W]: the disparity of the surface seen at each pixel of the view
              (of the source view's scale); NaN in an unfilled hole
      state   uint8 [B, H, W]: 0 = a surface was seen, 1 = hole (also where it was filled)
      source  float32 [B, H, W]: the source column, fractional, that is seen; -1 in a hole
    None differentiable."""


def forward_warp(image: torch.Tensor, disp: torch.Tensor, scale=1.0, exclude: torch.Tensor = None,
                 max_diff: float = 1.0, max_stretch: float = 4.0, fill: bool = True, fill_value: float = 0.0,
                 want_zview: bool = True, want_state: bool = True, want_source: bool = False) -> WarpedView:
    """``lea_forward_warp_f32`` (include/leastereo_hip.h): ``image`` [B, C, H, W] float32,
    C 1 .. 4, pushed forward through its own disparity ``disp`` [B, H, W] to where a camera
    ``scale`` baselines along sees it (source column x lands on x - scale * d), as a 1-D mesh per
    scanline: the nearest surface wins a pixel, neighbours further apart than ``max_diff`` px of
    disparity or stretched beyond ``max_stretch`` px are torn apart, and holes take the
    background beside them (``fill``) or ``fill_value``.  ``scale``: a Python float for every
    item or a [B] float32 device tensor, read on the device at every launch and replay.
    ``exclude``: [B, H, W] uint8 or bool, or None (``DisparityLR.state`` /
    ``DisparitySpeckle.state`` go as they are).  One launch on the current stream; nothing is
    read back.  Returns ``WarpedView``."""
    who = "forward_warp"
    _require_cuda(image, disp)
    if image.dtype != torch.float32 or disp.dtype != torch.float32:
        raise ValueError("forward_warp: image and disp must be float32")
    if image.dim() != 4 or disp.dim() != 3 or 0 in image.shape:
        raise ValueError(f"forward_warp: image must be [B, C, H, W] and disp [B, H, W], got "
                         f"{tuple(image.shape)} and {tuple(disp.shape)}")
    b, c, h, w = image.shape
    if tuple(disp.shape) != (b, h, w):
        raise ValueError(f"forward_warp: disp {tuple(disp.shape)} does not match image {tuple(image.shape)}")
    if not 1 <= c <= 4:
        raise ValueError(f"forward_warp: {c} channels, 1 .. 4 supported")
    if w > FORWARD_WARP_MAX_W:
        raise ValueError(f"forward_warp: width {w} is above the kernel's limit {FORWARD_WARP_MAX_W}")
    e = _exclude_u8(exclude, (b, h, w), who)
    _number(who, "max_diff", max_diff, "a finite number >= 0", lo=0, finite=True)
    _number(who, "max_stretch", max_stretch, "in 1 .. 64", lo=1, hi=64)
    _number(who, "fill_value", fill_value, "a number", bools=True)
    dev = image.device
    if isinstance(scale, torch.Tensor):
        if not scale.is_cuda or scale.dtype != torch.float32 or tuple(scale.shape) != (b,):
            raise ValueError(f"forward_warp: a tensor scale must be [{b}] float32 on the device")
        sc = scale.contiguous()
    elif isinstance(scale, (int, float)) and not isinstance(scale, bool):
        sc = torch.full((b,), float(scale), device=dev, dtype=torch.float32)
    else:
        raise ValueError(f"forward_warp: scale must be a number or a [{b}] float32 device tensor")
    image, ibs = _image_view(image)
    d, dbs = _plane_view(disp, "disp")
    e = _contiguous(e)
    out = torch.empty((b, c, h, w), device=dev, dtype=torch.float32)
    zview = torch.empty((b, h, w), device=dev, dtype=torch.float32) if want_zview else None
    state = torch.empty((b, h, w), device=dev, dtype=torch.uint8) if want_state else None
    source = torch.empty((b, h, w), device=dev, dtype=torch.float32) if want_source else None
    n = float(b * h * w)
    _launch("lea_forward_warp_f32", image.data_ptr(), ibs, d.data_ptr(), dbs, _ptr(e), sc.data_ptr(), b, c, h, w,
            float(max_diff), float(max_stretch), 1 if fill else 0, float(fill_value), out.data_ptr(), _ptr(zview),
            _ptr(state), _ptr(source),
            probe=lambda: _op_record("forward_warp", 20.0 * n, n * (
                4.0 * (2 * c + 1) + (1.0 if e is not None else 0.0) + (4.0 if want_zview else 0.0) +
                (1.0 if want_state else 0.0) + (4.0 if want_source else 0.0))))
    return WarpedView(out, zview, state, source)


# ------------------------------------------------------------------ bf16 path (c8)
# Activations: torch.bfloat16 [B, C/8, D, H, W, 8] ("c8": 8 channels per voxel word).

def c8_channels(t: torch.Tensor) -> int:
    return t.shape[1] * 8


def to_c8(x: torch.Tensor) -> torch.Tensor:
    """f32 [B, C, D, H, W] (or [B, C, H, W] as D = 1) -> bf16 c8."""
    _require_cuda(x)
    x5 = x.unsqueeze(2) if x.dim() == 4 else x
    b, c, d, h, w = x5.shape
    xbs = _check_volume_view(x5, "x")
    out = torch.empty((b, c // 8, d, h, w, 8), device=x.device, dtype=torch.bfloat16)
    _launch("lea_to_c8_bf16", x5.data_ptr(), xbs, out.data_ptr(), out.stride(0), b, c, d * h * w,
            probe=lambda: _op_record("to_c8_bf16", 0.0, 6.0 * out.numel()))
    return out


def from_c8(x: torch.Tensor) -> torch.Tensor:
    """bf16 c8 -> f32 [B, C, D, H, W]."""
    _require_c8(x)
    b, cb, d, h, w, _ = x.shape
    xbs = _check_c8_view(x, "x")
    out = torch.empty((b, cb * 8, d, h, w), device=x.device, dtype=torch.float32)
    _launch("lea_from_c8_bf16", x.data_ptr(), xbs, out.data_ptr(), out.stride(0), b, cb * 8, d * h * w)
    return out


def pack_conv_weight_bf16(w: torch.Tensor) -> torch.Tensor:
    """[cout, cin, k, k, k] f32 device weight -> packed bf16 fragments (bf16 engine)."""
    _require_cuda(w)
    w = w.detach().contiguous()
    cout, cin, k = w.shape[0], w.shape[1], w.shape[-1]
    n = _lib.load().lea_conv3d_packed_elems_bf16(cout, cin, k)
    if n == 0:
        raise ValueError(f"unsupported bf16 conv shape cout={cout} cin={cin} k={k}")
    packed = torch.empty(n, device=w.device, dtype=torch.bfloat16)
    _launch("lea_conv3d_pack_weights_bf16", w.data_ptr(), packed.data_ptr(), cout, cin, k)
    return packed


def conv_kernel_name_bf16(b, cout, cin, d, h, w, k, costvolume=False, cin2=0, flags=0):
    """The kernel of a bf16 conv launch (None where the launch refuses); cin2 of the cin input
    channels come from the second source, flags as the launch's (LEA_PAIR_SUM: the pair launch)."""
    return _decode(_lib.load().lea_conv3d_launch_kernel_name_bf16(b, cin, cin2, cout, d, h, w, k, flags,
                                                                  1 if costvolume else 0))


def conv3d_bnrelu_bf16(x: torch.Tensor, packed: torch.Tensor, cout: int, k: int,
                       scale: torch.Tensor | None, shift: torch.Tensor | None, relu: bool = True,
                       out: torch.Tensor | None = None, accumulate: bool = False,
                       x2: torch.Tensor | None = None,
                       residual: torch.Tensor | None = None, pair_sum: bool = False) -> torch.Tensor:
    """conv3d_bnrelu at dtype bf16 on c8 tensors (out may be a block slice).  ``pair_sum``
    (LEA_PAIR_SUM, the D-streaming kernel): x's and x2's channels feed two ConvBRs whose
    activations are summed; ``packed`` = pack_conv_weight_bf16(W_a) then (W_b) (one K chunk
    each), scale / shift 2 * cout values."""
    _require_c8(x, x2, out, residual)
    _require_cuda(scale, shift)
    if pair_sum and (x2 is None or accumulate or residual is not None):
        raise ValueError("pair_sum takes two sources and no residual")
    b, cb, d, h, w, _ = x.shape
    xbs = _check_c8_view(x, "x")
    x2ptr, x2bs, cin2 = _second_source(x2, b, (d, h, w), c8=True)
    cin = cb * 8 + cin2
    out, ybs = _conv_out(b, cout, (d, h, w), out, accumulate, x.device, c8=True)
    rptr, rbs = _residual(out, accumulate, residual, ybs, c8=True)
    _launch("lea_conv3d_bnrelu_bf16", x.data_ptr(), xbs, x2ptr, x2bs, cin2, packed.data_ptr(), _ptr(scale),
            _ptr(shift), rptr, rbs, out.data_ptr(), ybs, b, cin, cout, d, h, w, k,
            _flags(relu, rptr is not None, pair_sum),
            probe=lambda: _conv_record(
                b, cin, cout, d, h, w, k, rptr is not None, b * d * h * w, False,
                name=conv_kernel_name_bf16(b, cout, cin, d, h, w, k, cin2=cin2, flags=_flags(False, False, pair_sum)),
                esz=2))
    return out


def pair_sum_supported_bf16(x: torch.Tensor, x2: torch.Tensor, out: torch.Tensor) -> bool:
    """Whether conv3d_bnrelu_bf16(..., pair_sum=True) takes these c8 operands: two equal sources
    of one K chunk each (8 or 16 channels), cout <= 16, D >= 4 (the D-streaming kernel)."""
    if not (x.shape[1] == x2.shape[1] and tuple(x.shape[2:5]) == tuple(x2.shape[2:5])):
        return False
    # the library's own plan decides the rest (a tuning override can take the shape off the
    # D-streaming kernel): ask it rather than fail mid-forward
    b, cb, d, h, w = (int(s) for s in x.shape[:5])
    return bool(_lib.load().lea_conv3d_bf16_pair_supported(b, cb * 8, int(out.shape[1]) * 8, d, h, w))


def conv1x1_resampled_bf16(x: torch.Tensor, size, packed: torch.Tensor, cout: int, scale, shift,
                           relu: bool = True, out: torch.Tensor | None = None) -> torch.Tensor:
    """ConvBR 1x1 of interp(x, size, align_corners=True) on c8 tensors, the resampled
    input never materialised (lea_conv1x1_resampled_bf16)."""
    _require_c8(x, out)
    _require_cuda(scale, shift)
    b, cb, di, hi, wi, _ = x.shape
    d, h, w = (int(t) for t in size)
    xbs = _check_c8_view(x, "x")
    out, ybs = _conv_out(b, cout, (d, h, w), out, False, x.device, c8=True)
    _launch("lea_conv1x1_resampled_bf16", x.data_ptr(), xbs, di, hi, wi, packed.data_ptr(), _ptr(scale),
            _ptr(shift), out.data_ptr(), ybs, b, cb * 8, cout, d, h, w, _flags(relu),
            probe=lambda: _conv_record(b, cb * 8, cout, d, h, w, 1, False, b * di * hi * wi, True,
                                       name="conv1x1_rs_c8_kernel", esz=2))
    return out


def conv3d_bnrelu_costvolume_bf16(fl: torch.Tensor, fr: torch.Tensor, maxdisp: int,
                                  packed: torch.Tensor, cout: int, scale, shift,
                                  relu: bool = True) -> torch.Tensor:
    """conv3d_bnrelu_costvolume at bf16: fl/fr c8 feature maps [B, C/8, 1, H, W, 8]."""
    _require_c8(fl, fr)
    if fl.shape != fr.shape or fl.shape[2] != 1:
        raise ValueError("left/right c8 features must match and have D = 1")
    fbs = _check_c8_view(fl, "left")
    if _check_c8_view(fr, "right") != fbs:
        raise ValueError("left/right batch strides differ")
    b, cb, _, h, w, _ = fl.shape
    d3 = int(maxdisp / 3)
    out = torch.empty((b, cout // 8, d3, h, w, 8), device=fl.device, dtype=torch.bfloat16)
    _launch("lea_conv3d_bnrelu_costvolume_bf16", fl.data_ptr(), fr.data_ptr(), fbs, packed.data_ptr(), _ptr(scale),
            _ptr(shift), out.data_ptr(), out.stride(0), b, cb * 8, cout, d3, h, w, _flags(relu),
            probe=lambda: _conv_record(b, 2 * cb * 8, cout, d3, h, w, 3, False, 0, False,
                                       name=conv_kernel_name_bf16(b, cout, 2 * cb * 8, d3, h, w, 3, True), esz=2))
    return out


def resample_trilinear_bf16(x: torch.Tensor, size, align_corners: bool = True,
                            out: torch.Tensor | None = None, scale=None, shift=None,
                            relu: bool = False) -> torch.Tensor:
    """resample_trilinear on c8 tensors."""
    _require_c8(x, out)
    b, cb, di, hi, wi, _ = x.shape
    do, ho, wo = (int(s) for s in size)
    xbs = _check_c8_view(x, "x")
    out, ybs = _out_view(out, (b, cb, do, ho, wo, 8), x.device, c8=True)
    _launch("lea_resample3d_trilinear_bf16", x.data_ptr(), xbs, out.data_ptr(), ybs, b, cb * 8, di, hi, wi, do, ho,
            wo, 1 if align_corners else 0, _ptr(scale), _ptr(shift), _flags(relu),
            probe=lambda: _op_record("resample3d_c8", 0.0, 2.0 * b * cb * 8 * (di * hi * wi + do * ho * wo)))
    return out


def tapsum_upsample_bf16(q: torch.Tensor, cout: int, size, scale=None, shift=None,
                         relu: bool = False) -> torch.Tensor:
    """tapsum_upsample with q in c8 (27*cout channels padded to a multiple of 8) -> f32."""
    _require_c8(q)
    b, cb, di, hi, wi, _ = q.shape
    if cb * 8 < 27 * cout:
        raise ValueError(f"q has {cb * 8} channels, need 27*{cout}")
    return _tapsum(q, _check_c8_view(q, "q"), cout, (di, hi, wi), size, scale, shift, relu, LEA_BF16,
                   lambda out: _op_record("tapsum_c8", 0.0, 2.0 * q.numel() + 4.0 * out.numel()))


def pack_conv2d_weight_bf16(w: torch.Tensor) -> torch.Tensor:
    """[cout, cin, 3, 3] f32 device weight -> packed bf16 fragments (2D engine)."""
    w, cout, cin = _conv2d_weight(w)
    n = _lib.load().lea_conv2d_packed_elems_bf16(cout, cin)
    if n == 0:
        raise ValueError(f"unsupported bf16 conv2d shape cout={cout} cin={cin}")
    packed = torch.empty(n, device=w.device, dtype=torch.bfloat16)
    _launch("lea_conv2d_pack_weights_bf16", w.data_ptr(), packed.data_ptr(), cout, cin)
    return packed


def conv2d_bnrelu_bf16(x: torch.Tensor, packed: torch.Tensor, cout: int, scale, shift,
                       relu: bool = True, out: torch.Tensor | None = None, accumulate: bool = False,
                       residual: torch.Tensor | None = None) -> torch.Tensor:
    """conv2d_bnrelu on c8 maps [B, C/8, 1, H, W, 8]."""
    _require_c8(x, out, residual)
    _require_cuda(scale, shift)
    b, cb, d, h, w, _ = x.shape
    if d != 1:
        raise ValueError("conv2d_bnrelu_bf16 takes D = 1 maps")
    xbs = _check_c8_view(x, "x")
    out, ybs = _conv_out(b, cout, (1, h, w), out, accumulate, x.device, c8=True)
    rptr, rbs = _residual(out, accumulate, residual, ybs, c8=True)
    _launch("lea_conv2d_bnrelu_bf16", x.data_ptr(), xbs, packed.data_ptr(), _ptr(scale), _ptr(shift), rptr, rbs,
            out.data_ptr(), ybs, b, cb * 8, cout, h, w, _flags(relu, rptr is not None),
            probe=lambda: _op_record(
                "conv2d_bf16", 2.0 * b * h * w * cout * cb * 8 * 9,
                2.0 * b * h * w * (cb * 8 + cout * (2 if rptr is not None else 1)) + 18.0 * cout * cb * 8))
    return out


# ---- stem0 over the cost volume, factored through 2D maps (csrc/cv_stem.hip) ----

def cv_stem_split_weights(w: torch.Tensor):
    """stem0's [cout, 2C, 3, 3, 3] weight -> (wl [9 cout, C, 3, 3], wr [6 cout, C, 3, 3]),
    the 2D map weights of lea_cv_stem_split_weights."""
    _require_cuda(w)
    w = w.detach().contiguous()
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3) or w.shape[1] % 2:
        raise ValueError(f"expected a [cout, 2C, 3, 3, 3] weight, got {tuple(w.shape)}")
    cout, c = w.shape[0], w.shape[1] // 2
    wl = torch.empty((9 * cout, c, 3, 3), device=w.device, dtype=torch.float32)
    wr = torch.empty((6 * cout, c, 3, 3), device=w.device, dtype=torch.float32)
    _launch("lea_cv_stem_split_weights", w.data_ptr(), wl.data_ptr(), wr.data_ptr(), cout, c)
    return wl, wr


def cv_stem_map_windows(d3: int, w: int):
    """The columns of the maps that the f32 combine kernels read: (masked left maps' window,
    K2 maps' two windows), each (begin, end) (lea_cv_stem_map_windows)."""
    left, right = (ctypes.c_int * 2)(), (ctypes.c_int * 4)()
    check(_lib.load().lea_cv_stem_map_windows(d3, w, left, right), "lea_cv_stem_map_windows")
    return (left[0], left[1]), ((right[0], right[1]), (right[2], right[3]))


def cv_stem_supported(cout: int, d3: int, w: int, bf16: bool) -> bool:
    """Shapes lea_cv_stem_combine takes (f32 stores float4 rows; one plane has no
    interior to factor around)."""
    return d3 >= 2 and (cout % 8 == 0 if bf16 else w % 4 == 0)


def _cv_stem_maps(who, lmaps, rmaps, cout, c8=False):
    """The 2D maps of the factored stem0 in either layout: (B, H, W, left and right batch stride)."""
    (_require_c8 if c8 else _require_cuda)(lmaps, rmaps)
    b, h, w = lmaps.shape[0], lmaps.shape[3], lmaps.shape[4]
    lbs, rbs = _batch_stride(lmaps, "lmaps", c8), _batch_stride(rmaps, "rmaps", c8)
    per = 8 if c8 else 1
    if lmaps.shape[1] * per != 9 * cout or rmaps.shape[1] * per != 6 * cout:
        raise ValueError(f"{who}: map channels must be 9 / 6 x cout")
    return b, h, w, lbs, rbs


def cv_stem_combine(lmaps: torch.Tensor, rmaps: torch.Tensor, cout: int, d3: int,
                    scale: torch.Tensor | None, shift: torch.Tensor | None, relu: bool = True,
                    name: str = "cv_stem_f32_kernel", tmajor: bool = False) -> torch.Tensor:
    """stem0's output from the 2D maps: lmaps [B, 9 cout, 1, H, W] / rmaps [B, 6 cout, 1, H, W]
    f32 -> [B, cout, D3, H, W] f32, or c8 maps -> c8 [B, cout/8, D3, H, W, 8] bf16.  ``tmajor``
    (f32): lmaps in the order (3 t + kd) cout + o (LEA_CVS_TMAJOR)."""
    c8 = lmaps.dtype == torch.bfloat16
    b, h, w, lbs, rbs = _cv_stem_maps("cv_stem_combine", lmaps, rmaps, cout, c8)
    out = torch.empty(_act_shape(b, cout, (d3, h, w), c8), device=lmaps.device,
                      dtype=torch.bfloat16 if c8 else torch.float32)
    _require_cuda(scale, shift)
    if tuple(rmaps.shape[0:1]) != (b,) or tuple(rmaps.shape[3:5]) != (h, w):
        raise ValueError("cv_stem_combine: left/right maps differ in batch or size")
    # algorithmic bytes: the output write (the maps are L2/MALL-resident reads)
    _launch("lea_cv_stem_combine", lmaps.data_ptr(), lbs, rmaps.data_ptr(), rbs, _ptr(scale), _ptr(shift),
            out.data_ptr(), out.stride(0), b, cout, d3, h, w, _flags(relu) | (LEA_CVS_TMAJOR if tmajor else 0),
            LEA_BF16 if c8 else LEA_F32,
            probe=lambda: _op_record(name, 0.0, out.numel() * out.element_size(), 0.0,
                                     shape=(b, 0, cout, d3, h, w, 0)))
    return out


def cv_stem_down2_supported(lmaps: torch.Tensor, cout: int, d3: int) -> bool:
    """Whether cv_stem_combine_down2 takes these maps: f32 NCDHW maps on the device and a shape
    lea_cv_stem_down2_supported accepts (even D3 / H, W % 4 == 0, unsplit planes)."""
    if not lmaps.is_cuda or lmaps.dtype != torch.float32 or lmaps.dim() != 5:
        return False
    return bool(_lib.load().lea_cv_stem_down2_supported(cout, d3, lmaps.shape[3], lmaps.shape[4], LEA_F32))


def cv_stem_combine_down2(lmaps: torch.Tensor, rmaps: torch.Tensor, cout: int, d3: int,
                          scale: torch.Tensor | None, shift: torch.Tensor | None, relu: bool = True,
                          tmajor: bool = False):
    """``cv_stem_combine`` (f32) with stem0's output also at the next level: returns (y, y2),
    y2 [B, cout, D3/2, H/2, W/2] = resample_trilinear(y, (D3/2, H/2, W/2)) bit for bit, written
    by the same launch from the row pair it holds in registers (no second pass over y)."""
    _require_cuda(scale, shift)
    b, h, w, lbs, rbs = _cv_stem_maps("cv_stem_combine_down2", lmaps, rmaps, cout)
    if tuple(rmaps.shape[0:1]) != (b,) or tuple(rmaps.shape[3:5]) != (h, w):
        raise ValueError("cv_stem_combine_down2: left/right maps differ in batch or size")
    out = torch.empty((b, cout, d3, h, w), device=lmaps.device, dtype=torch.float32)
    out2 = torch.empty((b, cout, d3 // 2, h // 2, w // 2), device=lmaps.device, dtype=torch.float32)
    # algorithmic bytes: the maps and both outputs
    _launch("lea_cv_stem_combine_down2", lmaps.data_ptr(), lbs, rmaps.data_ptr(), rbs, _ptr(scale), _ptr(shift),
            out.data_ptr(), out.stride(0), out2.data_ptr(), out2.stride(0), b, cout, d3, h, w,
            _flags(relu) | (LEA_CVS_TMAJOR if tmajor else 0), LEA_F32,
            probe=lambda: _op_record("cv_stem_f32_down2_kernel", 0.0,
                                     4.0 * (lmaps.numel() + rmaps.numel() + out.numel() + out2.numel())))
    return out, out2


# ---- host steps either side of forward ----

def _require_u8_images(who, left, right):
    for t in (left, right):
        if not t.is_cuda or t.dtype != torch.uint8:
            raise _lib.HipKernelError(f"{who} needs uint8 device images, got {t.dtype} on {t.device}")


def standardize_crop_u8(left: torch.Tensor, right: torch.Tensor, crop_height: int, crop_width: int):
    """predict.py:162-184 (load_data) fused with :144-159 (test_transform) on the device.

    ``left``/``right``: uint8 [B, H, W, 3|4] (or [H, W, 3|4]) decoded images on the
    ROCm device.  Returns (left, right) float32 [B, 3, crop_height, crop_width]."""
    _require_u8_images("standardize_crop_u8", left, right)
    if left.dim() == 3:
        left, right = left.unsqueeze(0), right.unsqueeze(0)
    if left.shape != right.shape or left.dim() != 4 or left.shape[-1] not in (3, 4):
        raise ValueError(f"left/right must both be [B, H, W, 3|4] uint8, got {tuple(left.shape)} "
                         f"and {tuple(right.shape)}")
    left, right = left.contiguous(), right.contiguous()
    b, h, w, ps = left.shape
    lib = _lib.load()
    ws = torch.empty(lib.lea_standardize_workspace_bytes(b), device=left.device, dtype=torch.uint8)
    out_l = torch.empty((b, 3, crop_height, crop_width), device=left.device, dtype=torch.float32)
    out_r = torch.empty_like(out_l)
    rc = _call("lea_standardize_crop_u8", left.data_ptr(), right.data_ptr(), b, h, w, ps, out_l.data_ptr(),
               out_r.data_ptr(), crop_height, crop_width, ws.data_ptr())
    if rc == _lib.LEA_E_INVALID and b"test_transform" in lib.lea_last_error():
        raise ValueError(lib.lea_last_error().decode())
    check(rc, "lea_standardize_crop_u8")
    return out_l, out_r


def train_transform_u8(left: torch.Tensor, right: torch.Tensor, disp_left: torch.Tensor, disp_right,
                       params: torch.Tensor, crop_height: int, crop_width: int, maxdisp: float):
    """common.py:119-131 (set_rgb_layers) fused with :43-91 (train_transform) on the device.

    ``left``/``right``: uint8 [B, H, W, 3|4]; ``disp_left``/``disp_right``: float32 [B, H, W]
    (``disp_right`` may be None); ``params``: int32 [B, 5] rows of
    ``{src_y0, src_x0_left, src_x0_right, target_sub, flags}`` (``data.sample_train_params``),
    all on the ROCm device.  Returns (left, right float32 [B, 3, ch, cw], target float32
    [B, 1, ch, cw], n_valid int32 [B]).  Nothing is copied to the host and nothing
    synchronises: the launches read ``params`` from device memory, so the call can be
    captured in a graph and replayed after ``params`` is overwritten."""
    _require_u8_images("train_transform_u8", left, right)
    _require_cuda(disp_left, disp_right)
    if not params.is_cuda or params.dtype != torch.int32:
        raise _lib.HipKernelError(f"train_transform_u8 needs int32 device params, got "
                                  f"{params.dtype} on {params.device}")
    if left.shape != right.shape or left.dim() != 4 or left.shape[-1] not in (3, 4):
        raise ValueError(f"left/right must both be [B, H, W, 3|4] uint8, got {tuple(left.shape)} "
                         f"and {tuple(right.shape)}")
    b, h, w, ps = left.shape
    for d in (disp_left, disp_right):
        if d is not None and tuple(d.shape) != (b, h, w):
            raise ValueError(f"disparities must be [B, H, W] = {(b, h, w)}, got {tuple(d.shape)}")
    if tuple(params.shape) != (b, 5):
        raise ValueError(f"params must be [B, 5] = {(b, 5)}, got {tuple(params.shape)}")
    left, right, disp_left, params = left.contiguous(), right.contiguous(), disp_left.contiguous(), params.contiguous()
    disp_right = _contiguous(disp_right)
    dev = left.device
    ws = torch.empty(_lib.load().lea_train_transform_workspace_bytes(b), device=dev, dtype=torch.uint8)
    out_l = torch.empty((b, 3, crop_height, crop_width), device=dev, dtype=torch.float32)
    out_r = torch.empty_like(out_l)
    out_t = torch.empty((b, 1, crop_height, crop_width), device=dev, dtype=torch.float32)
    n_valid = torch.empty((b,), device=dev, dtype=torch.int32)
    _launch("lea_train_transform_u8", left.data_ptr(), right.data_ptr(), b, h, w, ps, disp_left.data_ptr(),
            _ptr(disp_right), params.data_ptr(), out_l.data_ptr(), out_r.data_ptr(), out_t.data_ptr(), crop_height,
            crop_width, float(maxdisp), n_valid.data_ptr(), ws.data_ptr())
    return out_l, out_r, out_t, n_valid


# ---- whole-scene inference: tile gather and blend (csrc/evalio.hip, csrc/tile_blend.hip) ----

def standardize_tiles_u8(left: torch.Tensor, right: torch.Tensor, origins: torch.Tensor, tile_height: int,
                         tile_width: int):
    """``lea_standardize_tiles_u8`` (include/leastereo_hip.h): one pair of uint8 scenes
    [H, W, 3|4] (or [1, H, W, 3|4]) cut into the N tiles whose (y, x) origins the int32 device
    tensor ``origins`` [N, 2] holds, standardised with the whole scene's statistics, 0 outside
    the scene.  Returns (left, right) float32 [N, 3, tile_height, tile_width].  Nothing is
    copied to the host and nothing synchronises; any origins are memory-safe."""
    _require_u8_images("standardize_tiles_u8", left, right)
    if not origins.is_cuda or origins.dtype != torch.int32:
        raise _lib.HipKernelError(f"standardize_tiles_u8 needs int32 device origins, got "
                                  f"{origins.dtype} on {origins.device}")
    if left.dim() == 4 and left.shape[0] == 1:
        left, right = left[0], right[0]
    if left.shape != right.shape or left.dim() != 3 or left.shape[-1] not in (3, 4):
        raise ValueError(f"left/right must both be [H, W, 3|4] uint8, got {tuple(left.shape)} "
                         f"and {tuple(right.shape)}")
    if origins.dim() != 2 or origins.shape[1] != 2 or origins.shape[0] < 1:
        raise ValueError(f"origins must be [N, 2] with N >= 1, got {tuple(origins.shape)}")
    left, right, origins = left.contiguous(), right.contiguous(), origins.contiguous()
    h, w, ps = left.shape
    n = origins.shape[0]
    ws = torch.empty(_lib.load().lea_standardize_tiles_workspace_bytes(), device=left.device, dtype=torch.uint8)
    out_l = torch.empty((n, 3, tile_height, tile_width), device=left.device, dtype=torch.float32)
    out_r = torch.empty_like(out_l)
    _launch("lea_standardize_tiles_u8", left.data_ptr(), right.data_ptr(), h, w, ps, origins.data_ptr(), n,
            out_l.data_ptr(), out_r.data_ptr(), tile_height, tile_width, ws.data_ptr())
    return out_l, out_r


def blend_tiles(tiles: torch.Tensor, plan, view: str = "left", check: bool = False,
                count: torch.Tensor = None) -> torch.Tensor:
    """``lea_tile_blend_f32`` (include/leastereo_hip.h): the per-tile maps ``tiles``
    [N, tile_h, tile_w] float32 of ``plan`` (a ``scene.TilePlan``; N = ny * nx, any batch
    stride) blended into one [H, W] map with the plan's weights.  ``view`` "left" for the
    left view's maps (disparity, entropy, peak, local disparity), "right" for the right view's
    disparity, whose truncated columns are on the tile's right.  ``count``: an int32 device
    tensor of one element that receives the number of pixels no tile covers.  ``check=True``
    reads that count back (a synchronisation) and raises if it is not 0; the default neither
    counts nor synchronises."""
    _require_cuda(tiles)
    n, th, tw = plan.ny * plan.nx, plan.tile_h, plan.tile_w
    if tiles.dim() != 3 or tuple(tiles.shape) != (n, th, tw):
        raise ValueError(f"tiles must be [N, tile_h, tile_w] = {(n, th, tw)}, got {tuple(tiles.shape)}")
    tiles, tbs = _plane_view(tiles, "tiles")
    (gy0, gy1), (gx0, gx1) = plan.guards(view)
    ys, xs = plan.device_axes(tiles.device)
    if check and count is None:
        count = torch.empty(1, device=tiles.device, dtype=torch.int32)
    if count is not None and (not count.is_cuda or count.dtype != torch.int32 or count.numel() != 1):
        raise ValueError("count must be one int32 element on the device")
    out = torch.empty((plan.height, plan.width), device=tiles.device, dtype=torch.float32)
    _launch("lea_tile_blend_f32", tiles.data_ptr(), tbs, ys.data_ptr(), plan.ny, xs.data_ptr(), plan.nx, th, tw,
            gy0, gy1, gx0, gx1, plan.ramp, out.data_ptr(), plan.height, plan.width, _ptr(count))
    if check:
        holes = int(count.item())
        if holes:
            raise _lib.HipKernelError(f"blend_tiles: {holes} of {plan.height * plan.width} pixels have no "
                                      f"covering tile (view {view!r})")
    return out


METRIC_FIELDS = ("n_epe", "sum_abs", "n_valid", "n_correct3", "n_le_thr1", "n_le_thr2", "n_le_thr3")


def disparity_metrics(pred: torch.Tensor, gt: torch.Tensor, maxdisp: float, round_pred: bool = False,
                      z_shift: int = 0, thresholds=(1, 2, 3), correct_mask: bool = False):
    """Per-pair metric counts of evaluation.py:287-307 / utils/metrics.py:6-46 in
    one device pass.  pred/gt: float32 [B, H, W] (or [H, W]) on the ROCm device.
    Returns (counts float64 [B, 8] on the device, laid out as
    ``include/leastereo_hip.h`` lea_disparity_metrics documents, and the uint8
    3-px correct mask [B, H, W] or None)."""
    _require_cuda(pred, gt)
    if pred.dim() == 2:
        pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
    if pred.shape != gt.shape or pred.dim() != 3:
        raise ValueError(f"pred/gt must both be [B, H, W], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if len(thresholds) != 3:
        raise ValueError("three bad-pixel thresholds")
    pred, gt = pred.contiguous(), gt.contiguous()
    b, h, w = pred.shape
    ws = torch.empty(_lib.load().lea_disparity_metrics_workspace_bytes(b, h, w), device=pred.device,
                     dtype=torch.uint8)
    out = torch.empty((b, 8), device=pred.device, dtype=torch.float64)
    mask = torch.empty((b, h, w), device=pred.device, dtype=torch.uint8) if correct_mask else None
    _launch("lea_disparity_metrics", pred.data_ptr(), h * w, gt.data_ptr(), h * w, b, h, w, float(maxdisp),
            int(bool(round_pred)), int(z_shift), *(int(t) for t in thresholds), _ptr(mask), out.data_ptr(),
            ws.data_ptr())
    return out, mask


# ---- Winograd F(2,3)-along-W 3x3x3 convs (csrc/conv3d_wino.hip), fp32 ----

def wino_eligible(cout: int, cin: int, k: int) -> bool:
    """Layers the Winograd engine takes: k = 3 and input channels in chunks of 4
    (couts <= 8 run depth-paired: the couts of two output planes in one 16-row tile)."""
    return k == 3 and cin % 4 == 0


# below this the direct engine's smaller tiles fill the chip better (A/B override:
# LEASTEREO_WINO_MIN_VOXELS)
WINO_MIN_VOXELS = int(os.environ.get("LEASTEREO_WINO_MIN_VOXELS", "200000"))
# ... except for 32-cout blocks on the one-barrier W x D tile down to this volume (r04
# planner audit, profiles/r04_planner_sweep.txt: the C2 L2 32->32 cells, 61 K voxels, 34.6 us
# on conv3d_wino2p_kernel vs 38.2 us direct; A/B override: LEASTEREO_WINO_SMALL32_MIN)
WINO_SMALL32_MIN = int(os.environ.get("LEASTEREO_WINO_SMALL32_MIN", "32768"))


def wino_preferred(b, cout, cin, d, h, w) -> bool:
    """Per-call engine choice for an eligible layer (tools/wino_sweep.py at config 2):
    Winograd wins on the large volumes when the output channels fill its 16/32/48-row
    blocks (stem0, stem1, conv1/2, the L1 cells and sibling groups, the 8->24 L0
    group); on the small L2 volumes only the 96-channel sibling groups gain, the
    32-channel cells take the pipelined W x D tile down to WINO_SMALL32_MIN voxels (r04)."""
    if b * d * h * w < WINO_MIN_VOXELS:
        # small volumes: only wide blocks amortise the tile; 32-cout blocks run the one-barrier
        # pipelined tile (more than two 4-channel chunks per depth pair)
        return cout % 32 == 0 and (cout >= 64 or (b * d * h * w >= WINO_SMALL32_MIN and cin > 8))
    return cout <= 8 or cout == 16 or cout == 24 or cout % 32 == 0 or cout % 48 == 0


def wino_mfma_scale(cout: int, name: str) -> float:
    """MFMA products issued per direct-convolution product: (F + 2) per 3F for the
    kernel's F (first template argument of ``name``), times the padding of cout to
    the engine's 16/32/48-row block.  The W x D engine (conv3d_wino2_kernel<Q, WC, MTE,
    ...>) issues 24 products per 72: 1/3, with couts padded to 16 WC MTE; the F(2,3) x F(2,3)
    tile (conv3d_wino22_kernel) 16 per 36: 4/9, couts padded to 16."""
    if name.startswith("conv3d_wino22_kernel"):  # F(2,3) x F(2,3): 16 per (2 x 2 outputs x 9 taps)
        return (-(-cout // 16) * 16) / cout * 4.0 / 9.0
    if name.startswith("conv3d_wino2p_kernel"):  # the one-barrier W x D tile: 32-cout blocks
        return (-(-cout // 32) * 32) / cout / 3.0
    if name.startswith("conv3d_wino44_kernel"):  # F(4,3) x F(4,3): 36 per (4 x 4 outputs x 9 taps)
        return (-(-cout // 32) * 32) / cout / 4.0
    if name.startswith("conv3d_wino2_kernel<"):
        _, wc, mte = (int(t) for t in name.split("<", 1)[1].split(",")[:3])
        cop = 16 * wc * mte
        return (-(-cout // cop) * cop) / cout / 3.0
    f = int(name.split("<", 1)[1].split(",", 1)[0])  # conv3d_wino_kernel<F, Q, MT, ...>
    if cout <= 8:  # depth-paired: 12 (plane, kh) steps per 9 taps, 16 rows = 8 couts x 2 planes
        return (f + 2) / (3.0 * f) * 12 / 9 * 8 / cout
    cop = 16 if cout <= 16 else (48 if cout % 32 != 0 and cout % 48 == 0 else 32)
    return (f + 2) / (3.0 * f) * (-(-cout // cop) * cop) / cout


@contextlib.contextmanager
def wino_depth_f2():
    """Run the enclosed Winograd convs of the pipelined kernel's layers on the F(4,3) x F(2,3)
    tile (lea_conv3d_wino44_set(0)) instead of the F(4,3) x F(4,3) one, then restore the
    setting the process had (_lib.tuning).  The training path uses it: its gradient
    bars (tests/test_gpu_training.py) were calibrated on the F(2,3)-along-D numerics, and
    F(4,3) along D adds fp32 roundings that the backward chain amplifies (r06: a feature-net
    BN-weight gradient at 2.9e-3 of its scale against the 2e-3 bar).  Process-wide, like
    every tuning setter: not for concurrent use from several threads."""
    with _lib.tuning(lea_conv3d_wino44_set=0):
        yield


def wino_kernel_name(b, cout, d, h, w, costvolume=False, cin=0):
    return _decode(_lib.load().lea_conv3d_wino_kernel_name(b, cin, cout, d, h, w, 1 if costvolume else 0))


def pack_conv_weight_wino(w: torch.Tensor) -> torch.Tensor:
    """[cout, cin, 3, 3, 3] fp32 device weight -> U = G g per kw row, the layout of
    lea_conv3d_bnrelu_wino."""
    _require_cuda(w)
    w = w.detach().contiguous()
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3):
        raise ValueError(f"expected a [cout, cin, 3, 3, 3] weight, got {tuple(w.shape)}")
    cout, cin = w.shape[0], w.shape[1]
    n = _lib.load().lea_conv3d_wino_packed_floats(cout, cin)
    if n == 0:
        raise ValueError(f"unsupported Winograd conv shape cout={cout} cin={cin}")
    packed = torch.empty(n, device=w.device, dtype=torch.float32)
    _launch("lea_conv3d_wino_pack_weights", w.data_ptr(), packed.data_ptr(), cout, cin)
    return packed


def pair_sum_supported(x: torch.Tensor, x2: torch.Tensor, out: torch.Tensor) -> bool:
    """Whether conv3d_bnrelu_wino(..., pair_sum=True) takes these operands: the F(2,3) x F(2,3)
    tile's rule (csrc/conv3d_wino22.hip wino22_ok) -- cout <= 32, W % 4 == 0, 16-byte aligned
    sources with batch strides of whole 16-byte words, 8-byte aligned output."""
    b, c, d, h, w = x.shape
    ok = out.shape[1] <= 32 and w % 4 == 0 and x2.shape[2:] == x.shape[2:] and x.shape[1] % 4 == 0
    for t, al in ((x, 16), (x2, 16), (out, 8)):
        ok = ok and t.data_ptr() % al == 0 and t.stride(0) % (al // 4) == 0 and \
            t.stride()[1:] == (d * h * w, h * w, w, 1)
    return bool(ok and 16 * d * h * w * 4 < 0xFFFFFF00)


def _wino_record(name, mfma_name, b, cin, cout, d, h, w, accumulate, in_vox, nbytes=None):
    """``_conv_record`` of a Winograd launch reported as ``name`` that issues the products of
    kernel ``mfma_name``."""
    return _conv_record(b, cin, cout, d, h, w, 3, accumulate, in_vox, False, name=name,
                        mfma_scale=wino_mfma_scale(cout, mfma_name), nbytes=nbytes)


def conv3d_bnrelu_wino(x: torch.Tensor, packed: torch.Tensor, cout: int,
                       scale: torch.Tensor | None, shift: torch.Tensor | None, relu: bool = True,
                       out: torch.Tensor | None = None, accumulate: bool = False,
                       x2: torch.Tensor | None = None,
                       residual: torch.Tensor | None = None, pair_sum: bool = False) -> torch.Tensor:
    """``conv3d_bnrelu`` (k = 3) on the Winograd engine: same semantics, weights
    packed by ``pack_conv_weight_wino``.  ``pair_sum`` (LEA_PAIR_SUM): x's and x2's channels
    feed two separate ConvBRs (the packed weight is [W_a | W_b] along cin, scale / shift
    2 * cout values) whose activations are summed -- a matching-cell step."""
    _require_cuda(x, x2, packed, scale, shift, out)
    if pair_sum and (x2 is None or accumulate or residual is not None):
        raise ValueError("pair_sum takes two sources and no residual")
    b, cin, d, h, w = x.shape
    xbs = _check_volume_view(x, "x")
    x2ptr, x2bs, cin2 = _second_source(x2, b, (d, h, w))
    out, ybs = _conv_out(b, cout, (d, h, w), out, accumulate, x.device)
    rptr, rbs = _residual(out, accumulate, residual, ybs)

    def probe():  # (the kernel-name query only when a probe listens)
        name = "conv3d_wino22_kernel" if pair_sum else wino_kernel_name(b, cout, d, h, w, cin=cin + cin2)
        return _wino_record(name, name, b, cin + cin2, cout, d, h, w, rptr is not None, b * d * h * w)

    _launch("lea_conv3d_bnrelu_wino", x.data_ptr(), xbs, x2ptr, x2bs, cin2, packed.data_ptr(), _ptr(scale),
            _ptr(shift), rptr, rbs, out.data_ptr(), ybs, b, cin + cin2, cout, d, h, w,
            _flags(relu, rptr is not None, pair_sum), LEA_F32, probe=probe)
    return out


def wino_down2_kernel_name(b, cin, cout, d, h, w, cin2=0):
    """The instantiation conv3d_bnrelu_wino_down2 launches for this shape (cin2 > 0: the
    two-input form, cin2 of the cin channels from x2), or None."""
    lib = _lib.load()
    return _decode(lib.lea_conv3d_wino_down2_cat_kernel_name(b, cin, cin2, cout, d, h, w) if cin2
                   else lib.lea_conv3d_wino_down2_kernel_name(b, cin, cout, d, h, w))


def conv3d_wino_down2_supported(x: torch.Tensor, cout: int) -> bool:
    """Whether conv3d_bnrelu_wino_down2 takes this input: an f32 NCDHW device tensor (16-byte
    aligned, whole 16-byte batch strides) of a shape the planner puts on the F(4,3) x F(4,3)
    tile (lea_conv3d_wino_down2_supported: even D / H, W % 4 == 0)."""
    return _wino_down2_supported(x, cout, None)


def conv3d_wino_down2_cat_supported(x: torch.Tensor, x2: torch.Tensor, cout: int) -> bool:
    """The same for cat(x, x2) read in place (lea_conv3d_wino_down2_cat_supported): both sources
    aligned, neither empty, channel counts in multiples of 4."""
    return _wino_down2_supported(x, cout, x2)


def _wino_down2_supported(x, cout, x2):
    if not all(_f32_volume(t, aligned=True) for t in ((x,) if x2 is None else (x, x2))):
        return False
    b, cin, d, h, w = x.shape
    if x2 is None:
        return bool(_lib.load().lea_conv3d_wino_down2_supported(b, cin, cout, d, h, w))
    if x2.shape[0] != b or tuple(x2.shape[2:]) != (d, h, w) or x2.device != x.device:
        return False
    return bool(_lib.load().lea_conv3d_wino_down2_cat_supported(b, cin + x2.shape[1], x2.shape[1], cout, d, h, w))


def conv3d_bnrelu_wino_down2(x: torch.Tensor, packed: torch.Tensor, cout: int,
                             scale: torch.Tensor | None, shift: torch.Tensor | None,
                             relu: bool = True) -> torch.Tensor:
    """resample_trilinear(conv3d_bnrelu_wino(x, ...), (D/2, H/2, W/2)) bit for bit, as one launch
    whose epilogue down-samples (the full-resolution output is never written)."""
    return _wino_down2(x, None, packed, cout, scale, shift, relu)


def conv3d_bnrelu_wino_down2_cat(x: torch.Tensor, x2: torch.Tensor, packed: torch.Tensor, cout: int,
                                 scale: torch.Tensor | None, shift: torch.Tensor | None,
                                 relu: bool = True) -> torch.Tensor:
    """The same on cat(x, x2) read in place, as conv3d_bnrelu_wino(x, ..., x2=x2) takes it
    (lea_conv3d_bnrelu_wino_down2_cat)."""
    return _wino_down2(x, x2, packed, cout, scale, shift, relu)


def _wino_down2(x, x2, packed, cout, scale, shift, relu):
    _require_cuda(x, x2, packed, scale, shift)
    b, cin, d, h, w = x.shape
    xbs = _check_volume_view(x, "x")
    x2ptr, x2bs, cin2 = _second_source(x2, b, (d, h, w))
    cin += cin2
    out = torch.empty((b, cout, d // 2, h // 2, w // 2), device=x.device, dtype=x.dtype)

    def probe():  # the same tile as the plain form; the bytes really moved: input + weights + the L1 output
        name = wino_down2_kernel_name(b, cin, cout, d, h, w, cin2) or (
            "conv3d_wino44_down2_cat_kernel" if cin2 else "conv3d_wino44_down2_kernel")
        return _wino_record(name, "conv3d_wino44_kernel", b, cin, cout, d, h, w, False, b * d * h * w,
                            nbytes=4.0 * (b * cin * d * h * w + out.numel()) + 4.0 * cout * cin * 27)

    if x2 is None:
        _launch("lea_conv3d_bnrelu_wino_down2", x.data_ptr(), xbs, packed.data_ptr(), _ptr(scale), _ptr(shift),
                out.data_ptr(), out.stride(0), b, cin, cout, d, h, w, _flags(relu), LEA_F32, probe=probe)
    else:
        _launch("lea_conv3d_bnrelu_wino_down2_cat", x.data_ptr(), xbs, x2ptr, x2bs, cin2, packed.data_ptr(),
                _ptr(scale), _ptr(shift), out.data_ptr(), out.stride(0), b, cin, cout, d, h, w, _flags(relu),
                LEA_F32, probe=probe)
    return out


def wino_dp_down2_kernel_name(b, cin, cout, d, h, w, only=False):
    """The instantiation conv3d_bnrelu_wino_dp_down2 launches for this shape, or None."""
    return _decode(_lib.load().lea_conv3d_wino_dp_down2_kernel_name(b, cin, cout, d, h, w, 1 if only else 0))


def conv3d_wino_dp_down2_supported(x: torch.Tensor, cout: int) -> bool:
    """Whether conv3d_bnrelu_wino_dp_down2 takes this input: an f32 NCDHW device tensor (16-byte
    aligned, whole 16-byte batch strides) of a shape the planner puts on a depth-paired tile
    (lea_conv3d_wino_dp_down2_supported: cout <= 8, even D / H, W % 4 == 0)."""
    if not _f32_volume(x, aligned=True):
        return False
    b, cin, d, h, w = x.shape
    return bool(_lib.load().lea_conv3d_wino_dp_down2_supported(b, cin, cout, d, h, w))


def conv3d_bnrelu_wino_dp_down2(x: torch.Tensor, packed: torch.Tensor, cout: int,
                                scale: torch.Tensor | None, shift: torch.Tensor | None, relu: bool,
                                out: torch.Tensor | None, down: torch.Tensor, accumulate: bool = False,
                                residual: torch.Tensor | None = None, only: bool = False) -> torch.Tensor:
    """conv3d_bnrelu_wino (couts <= 8: the depth-paired tiles) whose epilogue also writes ``down``
    [B, cout, D/2, H/2, W/2] = resample_trilinear(out, half), bit for bit.  ``only``: ``out`` is
    read as the residual (``accumulate``) but not written -- its final values never exist."""
    _require_cuda(x, packed, scale, shift, out, down, residual)
    b, cin, d, h, w = x.shape
    xbs = _check_volume_view(x, "x")
    if out is None:
        if not only or accumulate:
            raise ValueError("no out: the `only` form without accumulate")
        ybs = 0
    else:
        out, ybs = _conv_out(b, cout, (d, h, w), out, accumulate, x.device)
    down, dbs = _out_view(down, (b, cout, d // 2, h // 2, w // 2), x.device, name="down")
    rptr, rbs = _residual(out, accumulate, residual, ybs, shape=(b, cout, d, h, w))

    def probe():  # the bytes really moved: input, weights, residual, L0 output unless `only`, L1
        name = wino_dp_down2_kernel_name(b, cin, cout, d, h, w, only) or "conv3d_wino_dp_down2_kernel"
        vox = b * cout * d * h * w
        return _wino_record(
            name, wino_kernel_name(b, cout, d, h, w, cin=cin), b, cin, cout, d, h, w, rptr is not None,
            b * d * h * w, nbytes=4.0 * (x.numel() + (vox if rptr is not None else 0) + (0 if only else vox) +
                                         down.numel()) + 4.0 * cout * cin * 27)

    _launch("lea_conv3d_bnrelu_wino_dp_down2", x.data_ptr(), xbs, packed.data_ptr(), _ptr(scale), _ptr(shift),
            rptr, rbs, None if only else out.data_ptr(), ybs, down.data_ptr(), dbs, b, cin, cout, d, h, w,
            _flags(relu, rptr is not None), LEA_F32, probe=probe)
    return down


def conv3d_bnrelu_costvolume_wino(fl: torch.Tensor, fr: torch.Tensor, maxdisp: int,
                                  packed: torch.Tensor, cout: int, scale: torch.Tensor | None,
                                  shift: torch.Tensor | None, relu: bool = True) -> torch.Tensor:
    """``conv3d_bnrelu_costvolume`` on the Winograd engine (the cost volume of
    LEAStereo.py:34-48 read in place, never materialised)."""
    _require_cuda(fl, fr, packed, scale, shift)
    b, c, h, w = _feature_pair(fl, fr)
    d3 = int(maxdisp / 3)
    out = torch.empty((b, cout, d3, h, w), device=fl.device, dtype=fl.dtype)

    def probe():
        name = wino_kernel_name(b, cout, d3, h, w, True, cin=2 * c)
        return _wino_record(name, name, b, 2 * c, cout, d3, h, w, False, 0)

    _launch("lea_conv3d_bnrelu_costvolume_wino", fl.data_ptr(), fr.data_ptr(), fl.stride(0), packed.data_ptr(),
            _ptr(scale), _ptr(shift), out.data_ptr(), out.stride(0), b, c, cout, d3, h, w, _flags(relu), LEA_F32,
            probe=probe)
    return out
