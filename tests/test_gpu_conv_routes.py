"""The launches whose kernel the name queries used to get wrong (tests/test_conv_routes_cpu.py
lists the corrections), on the GPU: each runs the instantiation the query for the launch's whole
argument list names -- the probe record carries that name -- and computes, bit for bit, what the
same instantiation computes when a tuning hook selects it for operands the old query was right
about."""
import pytest
import torch

from leastereo_amd import _lib, kernels
from tests.test_conv_routes_cpu import PAIR_NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _c8(t):
    """f32 [B, C, D, H, W] on the device -> c8 bf16"""
    b, c, d, h, w = t.shape
    return t.reshape(b, c // 8, 8, d, h, w).permute(0, 1, 3, 4, 5, 2).contiguous().to(torch.bfloat16)


def _one(fn):
    with kernels.KernelProbe() as probe:
        out = fn()
    (rec,) = probe.records
    return rec.name, out


def test_bf16_two_sources_run_the_tile_kernel():
    """16 + 16 -> 16 channels at D >= 4: one source of 32 would stream; two stay on the tile."""
    g = torch.Generator().manual_seed(5)
    vol = (4, 8, 16)
    x = _c8(torch.randn(1, 32, *vol, generator=g).to(DEV))
    w = (torch.randn(16, 32, 3, 3, 3, generator=g) / 16).to(DEV)
    scale, shift = torch.rand(16, generator=g).to(DEV) + 0.5, torch.randn(16, generator=g).to(DEV)
    packed = kernels.pack_conv_weight_bf16(w)
    name, got = _one(lambda: kernels.conv3d_bnrelu_bf16(x[:, :2], packed, 16, 3, scale, shift, x2=x[:, 2:]))
    assert name == kernels.conv_kernel_name_bf16(1, 16, 32, *vol, 3, cin2=16)
    assert name.startswith("conv_bf16_kernel<3, 1, 1, 4, 2, 2,")
    assert kernels.conv_kernel_name_bf16(1, 16, 32, *vol, 3).startswith("conv_bf16_stream_kernel<")
    with _lib.tuning(lea_conv3d_bf16_set_variant=1):  # the materialised concat on the same tile
        name1, want = _one(lambda: kernels.conv3d_bnrelu_bf16(x, packed, 16, 3, scale, shift))
    assert name1 == name
    assert torch.equal(got, want)


def test_f32_resampled_1x1_beyond_the_gather_limit():
    """136 input channels: more than the gather-GEMM's LDS weight block holds."""
    g = torch.Generator().manual_seed(6)
    cin, cout, size = 136, 16, (1, 2, 4)
    x = torch.randn(1, cin, 2, 4, 8, generator=g).to(DEV)
    w = (torch.randn(cout, cin, 1, 1, 1, generator=g) / 8).to(DEV)
    scale, shift = torch.rand(cout, generator=g).to(DEV) + 0.5, torch.randn(cout, generator=g).to(DEV)
    packed = kernels.pack_conv_weight(w)
    name, got = _one(lambda: kernels.conv3d_bnrelu_resampled(x, size, packed, cout, 1, scale, shift))
    assert name == kernels.conv_kernel_name(1, cout, *size, 1, True, cin)
    assert name.startswith("conv3d_reg_kernel<1,")
    assert kernels.conv_kernel_name(1, cout, *size, 1, True) == "conv1x1_rs_f32_kernel<1>"
    with _lib.tuning(lea_conv3d_set_rs_gather=0):
        name0, want = _one(lambda: kernels.conv3d_bnrelu_resampled(x, size, packed, cout, 1, scale, shift))
    assert name0 == name
    assert torch.equal(got, want)


@pytest.mark.parametrize("cb", [1, 2])
@pytest.mark.parametrize("split", [0, 1, 2, 3])
def test_pair_launch_is_named_after_the_kernel_that_runs(split, cb):
    """lea_conv3d_bf16_set_pair_split flipped through _lib.tuning(), not the environment."""
    g = torch.Generator().manual_seed(7 + cb)
    c, vol = 8 * cb, (4, 8, 16)
    xa, xb = (_c8(torch.randn(1, c, *vol, generator=g).to(DEV)) for _ in range(2))
    packed = torch.cat([kernels.pack_conv_weight_bf16((torch.randn(c, c, 3, 3, 3, generator=g) / 8).to(DEV))
                        for _ in range(2)])
    scale, shift = torch.rand(2 * c, generator=g).to(DEV) + 0.5, torch.randn(2 * c, generator=g).to(DEV)
    with _lib.tuning(lea_conv3d_bf16_set_pair_split=split):
        name, _ = _one(lambda: kernels.conv3d_bnrelu_bf16(xa, packed, c, 3, scale, shift, x2=xb, pair_sum=True))
        assert name == kernels.conv_kernel_name_bf16(1, c, 2 * c, *vol, 3, cin2=c, flags=_lib.LEA_PAIR_SUM)
    assert name == PAIR_NAMES[split][cb]
