"""GPU checks of the down-sampling epilogues of the matching net's stems -- stem0's factored
kernel (csrc/cv_stem.hip, lea_cv_stem_combine_down2) and the F(4,3) x F(4,3) conv tile
(csrc/conv3d_wino44.hip, lea_conv3d_bnrelu_wino_down2) -- and of the executor route that uses
them.

The down-sampled output is the trilinear (align_corners) resample of the full output to half
the volume; for in == 2 out every output voxel reads one aligned 2 x 2 x 2 block, and the kernels
apply trilerp's own expression tree (common.h), so everything is compared with torch.equal:
stem0's y against lea_cv_stem_combine's and its y2 against lea_resample3d_trilinear of it, the
conv's output against lea_resample3d_trilinear of lea_conv3d_bnrelu_wino's.

Whole model: the 1x1 conv after the down-sampling moves from the register-staged resampling
engine to the streamed 1x1 kernel, whose sums associate differently, so fused against unfused
is held to the project's end-to-end bar (EPE < 1e-3 px, tests/test_gpu_parity.py
test_e2e_golden), as is the fused route against the reference's golden disparity."""

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, executor, kernels
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from oracle import torch_ref as ref
from tests.golden_util import golden, meta, normal, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
E2E_BAR = 1e-3  # px, test_e2e_golden's


def _maps(b, c, cout, maxdisp, hw, seed):
    g = torch.Generator().manual_seed(seed)
    fl = torch.randn((b, c) + hw, generator=g)
    fr = torch.randn((b, c) + hw, generator=g)
    w = torch.randn(cout, 2 * c, 3, 3, 3, generator=g) / np.sqrt(2 * c * 27)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(cout, generator=g) * 0.1).to(DEV)  # some outputs negative: the ReLU matters
    wl, wr = kernels.cv_stem_split_weights(w.to(DEV))
    lm = kernels.conv2d_bnrelu(fl.to(DEV).unsqueeze(2), kernels.pack_conv2d_weight(wl), 9 * cout, None,
                               None, relu=False)
    rm = kernels.conv2d_bnrelu(fr.to(DEV).unsqueeze(2), kernels.pack_conv2d_weight(wr), 6 * cout, None,
                               None, relu=False)
    return lm, rm, scale, shift


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("b,c,cout,maxdisp,hw", [
    (2, 32, 32, 48, (12, 40)),    # batch strides, a partial column segment
    (1, 8, 16, 12, (2, 8)),       # one row pair: every output is a last index on H
    (1, 32, 32, 192, (4, 100)),   # the benchmark's D3 = 64, two column segments, band and far lanes
    (1, 16, 24, 96, (6, 320))])   # a padded cout block, five segments
def test_cv_stem_down2_is_bit_identical(b, c, cout, maxdisp, hw, relu):
    lm, rm, scale, shift = _maps(b, c, cout, maxdisp, hw, c + cout + maxdisp)
    d3 = maxdisp // 3
    assert kernels.cv_stem_down2_supported(lm, cout, d3)
    want = kernels.cv_stem_combine(lm, rm, cout, d3, scale, shift, relu=relu)
    want2 = kernels.resample_trilinear(want, (d3 // 2, hw[0] // 2, hw[1] // 2))
    if relu:
        assert float((want == 0).float().mean()) > 0.05
    with kernels.KernelProbe() as probe:
        y, y2 = kernels.cv_stem_combine_down2(lm, rm, cout, d3, scale, shift, relu=relu)
    assert [r[0] for r in probe.records] == ["cv_stem_f32_down2_kernel"]
    assert probe.records[0][2] == 4.0 * (lm.numel() + rm.numel() + y.numel() + y2.numel())
    assert y2.shape == want2.shape
    assert torch.equal(y, want)
    assert torch.equal(y2, want2)


def test_cv_stem_down2_refuses_odd_and_split_shapes():
    lib = _lib.load()
    for cout, d3, hw in [(16, 5, (4, 8)),       # odd D3
                         (16, 4, (3, 8)),       # odd H
                         (8, 566, (2, 8))]:     # the planes split over two workgroups
        lm = torch.zeros(1, 9 * cout, 1, *hw, device=DEV)
        rm = torch.zeros(1, 6 * cout, 1, *hw, device=DEV)
        assert not kernels.cv_stem_down2_supported(lm, cout, d3)
        y = torch.full((1, cout, d3) + hw, 7.0, device=DEV)
        y2 = torch.full((1, cout, d3 // 2, hw[0] // 2, hw[1] // 2), 7.0, device=DEV)
        rc = lib.lea_cv_stem_combine_down2(lm.data_ptr(), lm.stride(0), rm.data_ptr(), rm.stride(0), None, None,
                                           y.data_ptr(), y.stride(0), y2.data_ptr(), y2.stride(0), 1, cout, d3,
                                           hw[0], hw[1], 0, _lib.LEA_F32, None)
        assert rc == 1002, (cout, d3, hw, rc)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()) and bool((y2 == 7.0).all())  # nothing launched
    assert not kernels.cv_stem_down2_supported(torch.zeros(1, 144, 1, 4, 8), 16, 4)  # not on the device
    assert not kernels.cv_stem_down2_supported(torch.zeros(1, 144, 1, 4, 8, device=DEV, dtype=torch.bfloat16), 16, 4)


# ------------------------------------------------- the F(4,3) x F(4,3) tile's DOWN epilogue
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("b,cin,cout,vol,walk", [
    (1, 32, 32, (4, 2, 32), 0),    # one tile; every output is a last index on H
    (1, 32, 32, (8, 4, 64), 0),    # two quads, two row tiles, two W tiles
    (2, 12, 32, (12, 6, 40), 0),   # batch strides, a partial W tile, three quads
    (1, 32, 24, (8, 4, 32), 0),    # padded cout block
    (1, 32, 32, (24, 4, 32), 3)])  # a forced multi-quad walk: the wait count after an epilogue
def test_wino44_down2_is_bit_identical(b, cin, cout, vol, walk, relu):
    lib = _lib.load()
    d, h, w = vol
    g = torch.Generator().manual_seed(cin + cout + d + h + w)
    x = torch.randn((b, cin) + vol, generator=g).to(DEV)
    wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) / np.sqrt(cin * 27)).to(DEV)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(cout, generator=g) * 0.3).to(DEV)  # some outputs negative: the ReLU matters
    packed = kernels.pack_conv_weight_wino(wt)
    with _lib.tuning(lea_conv3d_wino2_set_walk=walk):
        assert kernels.wino_kernel_name(b, cout, d, h, w, cin=cin) == "conv3d_wino44_kernel"
        assert kernels.conv3d_wino_down2_supported(x, cout)
        assert kernels.wino_down2_kernel_name(b, cin, cout, d, h, w) == "conv3d_wino44_down2_kernel"
        full = kernels.conv3d_bnrelu_wino(x, packed, cout, scale, shift, relu)
        want = kernels.resample_trilinear(full, (d // 2, h // 2, w // 2))
        with kernels.KernelProbe() as probe:
            got = kernels.conv3d_bnrelu_wino_down2(x, packed, cout, scale, shift, relu)
    assert [r[0] for r in probe.records] == ["conv3d_wino44_down2_kernel"]
    assert probe.records[0][2] == 4.0 * (x.numel() + got.numel() + cout * cin * 27)
    if relu:
        assert float((full == 0).float().mean()) > 0.05
    assert got.shape == want.shape
    assert torch.equal(got, want)


def test_wino44_down2_refuses_what_the_tile_does_not_take():
    x = torch.zeros(1, 32, 6, 4, 32, device=DEV)
    assert not kernels.conv3d_wino_down2_supported(x[:, :, :5], 32)  # odd D (and not contiguous)
    assert not kernels.conv3d_wino_down2_supported(x.cpu(), 32)
    assert not kernels.conv3d_wino_down2_supported(x, 16)  # the 16-cout layers run another tile
    assert kernels.wino_down2_kernel_name(1, 32, 16, 6, 4, 32) is None
    with _lib.tuning(lea_conv3d_wino44_set=0):  # the F(4,3) x F(2,3) tile: no DOWN form
        assert not kernels.conv3d_wino_down2_supported(x, 32)


# ---------------------------------------------------------------------- whole model
@pytest.fixture(scope="module")
def model():
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=48)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def _forward(m, left, right, fused):
    old = executor.MatchingExecutor.FUSED_DOWN
    executor.MatchingExecutor.FUSED_DOWN = fused
    try:
        with torch.no_grad(), kernels.KernelProbe() as probe:
            disp = m(left, right)
        return disp, [r[0] for r in probe.records]
    finally:
        executor.MatchingExecutor.FUSED_DOWN = old


def test_fused_route_runs_and_meets_the_e2e_bar(model):
    c = meta()["cases"]["e2e/b1_h96_w192_md48"]
    shape = (1, 3, c["height"], c["width"])
    left, right = normal(c["seeds"][0], shape).to(DEV), normal(c["seeds"][1], shape).to(DEV)
    fused, names = _forward(model, left, right, True)
    plain, names0 = _forward(model, left, right, False)
    # the fused launches replace the plain ones
    assert names.count("cv_stem_f32_down2_kernel") == 1 and "cv_stem_f32_kernel" not in names
    assert names0.count("cv_stem_f32_kernel") == 1 and "cv_stem_f32_down2_kernel" not in names0
    assert names.count("conv3d_wino44_down2_kernel") == 1 and "conv3d_wino44_down2_kernel" not in names0
    assert len(names) == len(names0)  # launch for launch: only what the four launches do changes
    g = golden("e2e")
    e32 = ref.epe(fused.cpu(), torch.from_numpy(g["b1_h96_w192_md48/disp32"]))
    e64 = ref.epe(fused.cpu(), torch.from_numpy(g["b1_h96_w192_md48/disp64"]))
    diff = ref.epe(fused.cpu(), plain.cpu())
    print(f"fused vs golden: EPE {e32:.3e} (f32) {e64:.3e} (f64) px; fused vs unfused: EPE {diff:.3e} px, "
          f"max {float((fused - plain).abs().max()):.3e} px")
    assert e32 < E2E_BAR and e64 < E2E_BAR, (e32, e64)
    assert diff < E2E_BAR, diff


def test_fused_route_batch_rows_are_independent(model):
    left = normal(901, (2, 3, 96, 192)).to(DEV)
    right = normal(902, (2, 3, 96, 192)).to(DEV)
    both, names = _forward(model, left, right, True)
    assert "cv_stem_f32_down2_kernel" in names and "conv3d_wino44_down2_kernel" in names
    one = torch.cat([_forward(model, left[i:i + 1], right[i:i + 1], True)[0] for i in range(2)])
    assert torch.equal(both, one)
    plain, _ = _forward(model, left, right, False)
    for i in range(2):
        assert ref.epe(both[i].cpu(), plain[i].cpu()) < E2E_BAR
