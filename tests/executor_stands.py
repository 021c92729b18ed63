"""torch stand-ins for the launches the executors issue, shared by the CPU tests of their graph
logic (tests/test_executor_plan_cpu.py, test_fanout_plan_cpu.py, test_down2_cpu.py,
test_executor_carry_cpu.py): the same contract as kernels.py (packed weights = the raw weights;
``out`` / ``accumulate`` / ``residual`` semantics) in plain torch ops, so that an executor runs in
float64 on CPU tensors and its graph logic is the only thing under test.  A test adds the launches
only its route issues on top of ``Stand`` (the two-head 1x1, the down-sampling epilogues)."""
import torch
import torch.nn.functional as F

from leastereo_amd import kernels


def _act(z, scale, shift, relu):
    if scale is not None:
        z = z * scale.view(1, -1, 1, 1, 1).to(z.dtype) + shift.view(1, -1, 1, 1, 1).to(z.dtype)
    return z.clamp_min(0) if relu else z


def _emit(y, out, accumulate=False, residual=None):
    if residual is not None:
        y = y + residual
    if out is None:
        return y
    if accumulate:
        out.add_(y)
    else:
        out.copy_(y)
    return out


class Stand:
    """torch stand-ins for the launches the f32 executors issue."""

    PACKERS = ("pack_conv_weight", "pack_conv2d_weight", "pack_conv_weight_wino")
    LAUNCHES = ("conv2d_bnrelu", "conv2d_bnrelu_pair", "conv2d_s3_bnrelu", "conv3d_bnrelu",
                "conv3d_bnrelu_resampled", "conv3d_bnrelu_wino", "resample_trilinear", "tapsum_upsample")

    def __init__(self):
        self.log = []     # ("conv2d", out ptr, accumulate), ("pair", out1 ptr, out2 ptr),
        #                   ("wino", out ptr, accumulate, pair_sum), and what a subclass adds
        self.single = []  # (source data_ptr, cout) of every single 1x1 launch at the source's size

    def install(self, monkeypatch, extra=()):
        """Put the stand-ins (and the subclass's ``extra`` ones) in place of kernels.*"""
        for name in self.PACKERS:
            monkeypatch.setattr(kernels, name, self.pack)
        for name in self.LAUNCHES + tuple(extra):
            monkeypatch.setattr(kernels, name, getattr(self, name))
        return self

    @staticmethod
    def pack(w):
        return w.detach().clone()

    def conv2d_bnrelu(self, x, packed, cout, scale, shift, relu=True, out=None, accumulate=False,
                      residual=None):
        self.log.append(("conv2d", out.data_ptr() if out is not None else None, accumulate))
        z = F.conv2d(x[:, :, 0], packed.to(x.dtype), padding=1).unsqueeze(2)
        return _emit(_act(z, scale, shift, relu), out, accumulate, residual)

    def conv2d_bnrelu_pair(self, x, packed, c1, cout, scale, shift, relu, out1, out2, residual=None):
        self.log.append(("pair", out1.data_ptr(), out2.data_ptr()))
        y = _act(F.conv2d(x[:, :, 0], packed.to(x.dtype), padding=1).unsqueeze(2), scale, shift, relu)
        _emit(y[:, :c1], out1, False, residual)
        _emit(y[:, c1:], out2, False, None)

    def conv2d_s3_bnrelu(self, x, w, scale, shift, relu=True):
        z = F.conv2d(x[:, :, 0], w.to(x.dtype), stride=3, padding=1).unsqueeze(2)
        return _act(z, scale, shift, relu)

    def conv3d_bnrelu(self, x, packed, cout, k, scale, shift, relu=True, out=None, accumulate=False,
                      x2=None, residual=None):
        if k == 1:
            self.single.append((x.data_ptr(), cout))
        if x2 is not None:
            x = torch.cat((x, x2), 1)
        z = F.conv3d(x, packed.to(x.dtype), padding=k // 2)
        return _emit(_act(z, scale, shift, relu), out, accumulate, residual)

    def conv3d_bnrelu_resampled(self, x, size, packed, cout, k, scale, shift, relu=True, out=None,
                                accumulate=False):
        x = F.interpolate(x, size=tuple(size), mode="trilinear", align_corners=True)
        z = F.conv3d(x, packed.to(x.dtype), padding=k // 2)
        return _emit(_act(z, scale, shift, relu), out, accumulate)

    def conv3d_bnrelu_wino(self, x, packed, cout, scale, shift, relu=True, out=None, accumulate=False,
                           x2=None, residual=None, pair_sum=False):
        self.log.append(("wino", out.data_ptr() if out is not None else None, accumulate, pair_sum))
        if not pair_sum:
            return self.conv3d_bnrelu(x, packed, cout, 3, scale, shift, relu, out, accumulate, x2, residual)
        ca = x.shape[1]
        ya = _act(F.conv3d(x, packed[:, :ca].to(x.dtype), padding=1), scale[:cout], shift[:cout], relu)
        yb = _act(F.conv3d(x2, packed[:, ca:].to(x.dtype), padding=1), scale[cout:], shift[cout:], relu)
        return _emit(ya + yb, out, False, None)

    def tapsum_upsample(self, q, cout, size, scale=None, shift=None, relu=False):
        """sum over the 27 taps of the up-sampled per-tap partial sums, shifted by the tap
        (channel co * 27 + tap): conv3x3x3(upsample(y)) by linearity."""
        assert cout == 1
        d, h, w = (int(v) for v in size)
        up = F.pad(F.interpolate(q, size=(d, h, w), mode="trilinear", align_corners=True), (1, 1, 1, 1, 1, 1))
        y = sum(up[:, (kd * 3 + kh) * 3 + kw::27][:, :1, kd:kd + d, kh:kh + h, kw:kw + w]
                for kd in range(3) for kh in range(3) for kw in range(3))
        return _act(y, scale, shift, relu)

    def resample_trilinear(self, x, size, align_corners=True, out=None, scale=None, shift=None,
                           relu=False):
        y = _act(F.interpolate(x, size=tuple(size), mode="trilinear", align_corners=align_corners),
                 scale, shift, relu)
        return _emit(y, out, False, None)
