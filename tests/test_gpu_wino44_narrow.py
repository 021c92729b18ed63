"""The 16 x 4 geometry of the F(4,3) x F(4,3) tile (csrc/conv3d_wino44.hip, w44::Geo<4>,
lea_conv3d_wino44_set_tile) against the 32 x 2 one.

Every voxel's arithmetic is the same in both geometries -- the same transforms, the same chunk
order, and an MFMA column's sum does not depend on which column it is -- so the outputs are
compared with torch.equal.  Each output is written into a channel slice between NaN sentinel
slices that must stay NaN.  Shapes: the smallest at which a geometry can go wrong (ragged in every
axis, less than one tile, one live group in the second tile column, exactly one tile column, the
C2 quarter-resolution width 80, three cout blocks, two chunks with a partial cout block, two
sources, batch 2).  Then the narrow tile against float64 torch at the project's conv bar, against
the float32 judge (tests/f32_judge.py) under the rule of tests/test_gpu_f32_numerics.py, and the
whole model with the tile forced wide and on auto."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from leastereo_amd import _lib, kernels
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from tests import f32_judge as J
from tests.golden_util import normal, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

# case: (batch, cin, first source's channels, cout, (D, H, W))
CASES = {
    "a": (1, 32, 32, 32, (5, 6, 20)),
    "b": (1, 32, 32, 32, (3, 3, 12)),
    "c": (1, 32, 32, 32, (8, 7, 80)),
    "d": (1, 32, 32, 96, (4, 9, 36)),
    "e": (1, 8, 8, 24, (6, 5, 84)),
    "f": (1, 16, 16, 32, (7, 8, 16)),
    "g": (1, 128, 64, 64, (4, 4, 16)),
    "h": (2, 32, 32, 32, (5, 6, 20)),
}


def _operands(case):
    b, cin, c1, cout, vol = CASES[case]
    g = torch.Generator().manual_seed(44 + cin + 3 * cout + vol[2])
    x = torch.randn((b, cin) + vol, generator=g).to(DEV)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / np.sqrt(cin * 27)).to(DEV)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    res = torch.randn((b, cout) + vol, generator=g).to(DEV)
    x1, x2 = (x[:, :c1].contiguous(), x[:, c1:].contiguous()) if c1 < cin else (x, None)
    return x, x1, x2, w, kernels.pack_conv_weight_wino(w), scale, shift, res


def _run(case, ops, tile, relu, resid, affine, walk=0, group=-1):
    """The layer into channels [8, 8 + cout) of a NaN-filled buffer with the tile forced; returns
    the slice (a copy) after checking the sentinel channels."""
    lib = _lib.load()
    b, cin, _, cout, vol = CASES[case]
    _, x1, x2, _, pw, scale, shift, res = ops
    big = torch.full((b, cout + 16) + vol, float("nan"), device=DEV)
    y = big[:, 8:8 + cout]
    with _lib.tuning(lea_conv3d_wino44_set_tile=tile, lea_conv3d_wino2_set_walk=walk,
                     lea_conv3d_wino44_set_group=group):
        assert kernels.wino_kernel_name(b, cout, *vol, cin=cin) == "conv3d_wino44_kernel"
        assert lib.lea_conv3d_wino44_tile(b, cin, cout, *vol) == tile
        if resid == "acc":
            y.copy_(res)
        kernels.conv3d_bnrelu_wino(x1, pw, cout, scale if affine else None, shift if affine else None, relu=relu,
                                   out=y, accumulate=resid == "acc", x2=x2,
                                   residual=res if resid == "res" else None)
    assert bool(big[:, :8].isnan().all()) and bool(big[:, 8 + cout:].isnan().all()), "sentinel channels written"
    return y.clone()


def _ref64(case, ops, relu, resid, affine):
    x, _, _, w, _, scale, shift, res = ops
    y = F.conv3d(x.double(), w.double(), None, 1, 1)
    if affine:
        y = y * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)
    if relu:
        y = y.relu()
    return y + res.double() if resid else y


FLAGS = list(itertools.product((True, False), (None, "res", "acc"), (True, False)))


@pytest.mark.parametrize("case", ["a", "d"])
def test_narrow_tile_writes_the_wide_tiles_bits_under_every_flag(case):
    """ReLU on / off x no residual / a residual / the accumulating form x scale and shift set /
    null, each with walks 1, 2 and auto and workgroup orders 0 and 3, on both tiles: all of them
    the bits of the wide tile at its default walk and order."""
    ops = _operands(case)
    for relu, resid, affine in FLAGS:
        wide = _run(case, ops, 32, relu, resid, affine)
        assert bool(torch.isfinite(wide).all())
        for walk, group in ((0, -1), (1, 0), (2, 0), (0, 3), (1, 3), (2, 3)):
            for tile in (16, 32):
                got = _run(case, ops, tile, relu, resid, affine, walk, group)
                assert torch.equal(got, wide), (case, tile, relu, resid, affine, walk, group)


@pytest.mark.parametrize("case,resid", [("b", "res"), ("c", "acc"), ("e", "acc"), ("f", "res"), ("g", "res"),
                                        ("h", "acc")])
def test_narrow_tile_writes_the_wide_tiles_bits(case, resid):
    ops = _operands(case)
    for rs in (None, resid):
        wide = _run(case, ops, 32, True, rs, True)
        narrow = _run(case, ops, 16, True, rs, True)
        assert bool(torch.isfinite(wide).all())
        assert torch.equal(narrow, wide), (case, rs)


@pytest.mark.parametrize("case", sorted(CASES))
def test_narrow_tile_vs_float64(case):
    """|d| <= 1e-4 + 1e-4 |ref|, the fp32 conv engines' bar (tests/test_gpu_wino.py)."""
    ops = _operands(case)
    got = _run(case, ops, 16, True, "res", True)
    want = _ref64(case, ops, True, "res", True)
    np.testing.assert_allclose(got.cpu().double().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("key,mode", [("c32x32", 1), ("c16x16", 3)])
def test_narrow_tile_error_is_within_four_times_its_model(key, mode):
    """E <= 4 x max(E(wino_f32(4, 4)), E(direct_f32)) on the judge's inputs: Judged.bar."""
    lib = _lib.load()
    failures = []
    with _lib.tuning(lea_conv3d_wino44_set=mode, lea_conv3d_wino44_set_tile=16):
        for case, seed in J.INPUT_SETS:
            j = J.judged(key, case, seed)
            x, w = torch.from_numpy(j.x).to(DEV), torch.from_numpy(j.w).to(DEV)
            cout, cin = w.shape[0], w.shape[1]
            assert kernels.wino_kernel_name(x.shape[0], cout, *x.shape[2:], cin=cin) == "conv3d_wino44_kernel"
            assert lib.lea_conv3d_wino44_tile(x.shape[0], cin, cout, *x.shape[2:]) == 16
            y = kernels.conv3d_bnrelu_wino(x, kernels.pack_conv_weight_wino(w), cout, None, None, relu=False)
            y = y.cpu().numpy()
            assert np.isfinite(y).all(), (key, case, seed)
            e, _ = j.error(y)
            bar = j.bar("wino44")
            print(f"w44 narrow {key} {case} s{seed}: E {e:.2e} model {j.e['wino44'][0]:.2e} "
                  f"direct {j.e['direct'][0]:.2e} bar {bar:.2e}")
            if not e <= bar:
                failures.append((case, seed, e, bar))
    assert not failures, (key, failures)


@pytest.mark.parametrize("height,width,maxdisp", [(96, 192, 48), (288, 576, 96)])
def test_disparity_is_equal_with_the_tile_wide_and_auto(height, width, maxdisp):
    """The whole model with lea_conv3d_wino44_set_tile(32) and on auto.  At 288 x 576 the
    quarter-resolution volumes are 48 wide: 3 narrow tiles or 1.5 wide ones, so auto takes the
    narrow geometry there."""
    lib = _lib.load()
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=maxdisp)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    m = m.to(DEV).eval()
    left, right = normal(931, (1, 3, height, width)).to(DEV), normal(932, (1, 3, height, width)).to(DEV)
    out = {}
    for tile in (32, -1):
        with _lib.tuning(lea_conv3d_wino44_set_tile=tile):
            with torch.no_grad(), kernels.KernelProbe() as probe:
                out[tile] = m(left, right)
            shapes = [r.shape for r in probe.records if r.name == "conv3d_wino44_kernel"]
            tiles = {lib.lea_conv3d_wino44_tile(*s[:6]) for s in shapes}
            assert shapes and 0 not in tiles
            if tile == 32:
                assert tiles == {32}
            elif width == 576:
                assert (1, 32, 96, 8, 24, 48) in [tuple(s[:6]) for s in shapes] and tiles == {16, 32}
                assert lib.lea_conv3d_wino44_tile(1, 32, 96, 8, 24, 48) == 16
    assert not out[32].isnan().any()
    assert torch.equal(out[-1], out[32])
