"""GPU checks of the down-sampling epilogues inside the matching net's cell chain: conv1 (the
F(4,3) x F(4,3) tile's DOWN form on cat(x, x2) read in place, lea_conv3d_bnrelu_wino_down2_cat)
and cell 10's output (the depth-paired Winograd tiles' DOWN forms, lea_conv3d_bnrelu_wino_dp_down2,
and s1's level-down copy, lea_resample3d_trilinear_down2), and of the executor routes that use them
(MatchingExecutor.FUSED_DOWN_CELLS).

As in tests/test_gpu_down2.py the down-sampled output is the trilinear (align_corners) resample
of the plain launch's output to half the volume, by trilerp's own expression tree, so every
kernel comparison is torch.equal.  Whole model: cells.5.share and cell 11's preprocess move from
the resampling engines to the streamed 1x1 kernel one level down, whose sums associate
differently, so on against off is held to the project's end-to-end bar (EPE < 1e-3 px, test_e2e_golden)."""
from collections import Counter

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


# ------------------------------------------- the F(4,3) x F(4,3) tile's DOWN epilogue, two inputs
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("b,cin1,cin2,cout,vol", [
    (1, 16, 16, 32, (4, 2, 32)),    # one tile; every output is a last index on H
    (2, 8, 24, 32, (8, 4, 64)),     # batch strides, two quads, two row tiles, two W tiles
    (1, 12, 20, 24, (8, 4, 32))])   # a padded cout block, sources that split off a chunk boundary of 8
def test_wino44_down2_cat_is_bit_identical(b, cin1, cin2, cout, vol, relu):
    d, h, w = vol
    cin = cin1 + cin2
    g = torch.Generator().manual_seed(cin1 + 3 * cin2 + cout + d + h + w)
    # both sources as channel slices of larger tensors, as the executor hands them over
    xa = torch.randn((b, cin1 + 8) + vol, generator=g).to(DEV)[:, 8:]
    xb = torch.randn((b, cin2 + 4) + vol, generator=g).to(DEV)[:, :cin2]
    wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) / np.sqrt(cin * 27)).to(DEV)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(cout, generator=g) * 0.3).to(DEV)  # some outputs negative: the ReLU matters
    packed = kernels.pack_conv_weight_wino(wt)
    assert kernels.wino_kernel_name(b, cout, d, h, w, cin=cin) == "conv3d_wino44_kernel"
    assert kernels.conv3d_wino_down2_cat_supported(xa, xb, cout)
    assert kernels.wino_down2_kernel_name(b, cin, cout, d, h, w, cin2) == "conv3d_wino44_down2_cat_kernel"
    # the one-input entry and its name are unchanged
    assert kernels.wino_down2_kernel_name(b, cin, cout, d, h, w) == "conv3d_wino44_down2_kernel"
    full = kernels.conv3d_bnrelu_wino(xa, packed, cout, scale, shift, relu, x2=xb)
    want = kernels.resample_trilinear(full, (d // 2, h // 2, w // 2))
    with kernels.KernelProbe() as probe:
        got = kernels.conv3d_bnrelu_wino_down2_cat(xa, xb, packed, cout, scale, shift, relu)
    assert [r[0] for r in probe.records] == ["conv3d_wino44_down2_cat_kernel"]
    assert probe.records[0][2] == 4.0 * (xa.numel() + xb.numel() + got.numel() + cout * cin * 27)
    if relu:
        assert float((full == 0).float().mean()) > 0.05
    assert got.shape == want.shape
    assert torch.equal(got, want)
    # one input through the same wrapper: the one-input launch, the same bits as the cat of both
    xc = torch.cat((xa, xb), 1)
    with kernels.KernelProbe() as probe:
        one = kernels.conv3d_bnrelu_wino_down2(xc, packed, cout, scale, shift, relu)
    assert [r[0] for r in probe.records] == ["conv3d_wino44_down2_kernel"]
    assert torch.equal(one, want)


def test_wino44_down2_cat_refuses_what_the_tile_does_not_take():
    lib = _lib.load()
    x = torch.zeros(1, 16, 4, 4, 32, device=DEV)
    assert kernels.conv3d_wino_down2_cat_supported(x, x, 32)
    assert not kernels.conv3d_wino_down2_cat_supported(x, x[:, :, :2], 32)       # volumes differ
    assert not kernels.conv3d_wino_down2_cat_supported(x, x.cpu(), 32)
    assert not kernels.conv3d_wino_down2_cat_supported(x, x.to(torch.bfloat16), 32)
    assert not kernels.conv3d_wino_down2_cat_supported(x, x[:, :6], 32)          # a chunk would straddle the sources
    assert not kernels.conv3d_wino_down2_cat_supported(x, x, 16)                 # the 16-cout layers run another tile
    assert not kernels.conv3d_wino_down2_cat_supported(x[:, :, :, :3], x[:, :, :, :3], 32)  # odd H
    assert kernels.wino_down2_kernel_name(1, 32, 32, 4, 4, 32, 6) is None
    assert kernels.wino_down2_kernel_name(1, 32, 32, 4, 4, 32, 32) is None   # nothing left for the first source
    # a refused entry launches nothing
    y = torch.full((1, 16, 2, 2, 16), 7.0, device=DEV)
    wp = torch.zeros(lib.lea_conv3d_wino_packed_floats(16, 32), device=DEV)
    rc = lib.lea_conv3d_bnrelu_wino_down2_cat(x.data_ptr(), x.stride(0), x.data_ptr(), x.stride(0), 16,
                                              wp.data_ptr(), None, None, y.data_ptr(), y.stride(0), 1, 32, 16,
                                              4, 4, 32, 0, _lib.LEA_F32, None)
    assert rc == 1002, rc
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ------------------------------------------------- the depth-paired tiles' DOWN epilogue
DP_SHAPES = [
    (1, 8, 8, (2, 4, 64), 0),     # one tile, one depth pair: every L1 index is a last index on D
    (1, 8, 8, (4, 8, 128), 0),    # two of everything
    (2, 8, 8, (6, 4, 96), 0),     # batch strides, a partial W tile (the 32-wide row pairs: Q = 8)
    (1, 8, 8, (12, 4, 64), 3),    # a multi-pair walk: the waits and the LDS exchange across items
    (1, 4, 8, (4, 4, 64), 0),     # one chunk: an epilogue every item
    (2, 8, 8, (4, 4, 64), 0)]     # batch strides on the 64-wide tile


@pytest.fixture(scope="module")
def dp_case():
    """Per (shape, relu): the operands, the plain accumulate launch's output and its resample,
    computed once for the side and the only form."""
    memo = {}

    def get(b, cin, cout, vol, walk, relu):
        key = (b, cin, cout, vol, walk, relu)
        if key not in memo:
            lib = _lib.load()
            d, h, w = vol
            g = torch.Generator().manual_seed(cin + cout + d + h + w)
            x = torch.randn((b, cin) + vol, generator=g).to(DEV)
            wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) / np.sqrt(cin * 27)).to(DEV)
            scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
            shift = (torch.randn(cout, generator=g) * 0.3).to(DEV)  # some outputs negative: the ReLU matters
            # the partial sums the launch accumulates onto: a channel slice, as a cell's slot is
            partial = torch.randn((b, cout + 8) + vol, generator=g).to(DEV)
            packed = kernels.pack_conv_weight_wino(wt)
            with _lib.tuning(lea_conv3d_wino2_set_walk=walk):
                act = kernels.conv3d_bnrelu_wino(x, packed, cout, scale, shift, relu)
                full = partial.clone()
                kernels.conv3d_bnrelu_wino(x, packed, cout, scale, shift, relu, out=full[:, 8:], accumulate=True)
            if relu:
                assert float((act == 0).float().mean()) > 0.05
            want = kernels.resample_trilinear(full[:, 8:], (d // 2, h // 2, w // 2))
            memo[key] = (x, packed, scale, shift, partial, full, want)
        return memo[key]
    return get


@pytest.mark.parametrize("only", [False, True], ids=["side", "only"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("b,cin,cout,vol,walk", DP_SHAPES)
def test_dp_down2_is_bit_identical(dp_case, b, cin, cout, vol, walk, relu, only):
    lib = _lib.load()
    d, h, w = vol
    x, packed, scale, shift, partial, full, want = dp_case(b, cin, cout, vol, walk, relu)
    q = 16 if kernels.wino_kernel_name(b, cout, d, h, w, cin=cin).startswith("conv3d_wino_kernel<4, 16, 0,") else 8
    assert (q == 8) == (w == 96)
    assert kernels.conv3d_wino_dp_down2_supported(x, cout)
    name = f"conv3d_wino_dp_down2_kernel<{q}, {'true' if only else 'false'}>"
    assert kernels.wino_dp_down2_kernel_name(b, cin, cout, d, h, w, only) == name
    y = partial.clone()
    down = torch.full((b, cout + 8, d // 2, h // 2, w // 2), 7.0, device=DEV)
    with _lib.tuning(lea_conv3d_wino2_set_walk=walk), kernels.KernelProbe() as probe:
        kernels.conv3d_bnrelu_wino_dp_down2(x, packed, cout, scale, shift, relu, y[:, 8:], down[:, :cout],
                                            accumulate=True, only=only)
    assert [r[0] for r in probe.records] == [name]
    assert torch.equal(down[:, :cout], want)
    assert bool((down[:, cout:] == 7.0).all())   # nothing past the slice
    # side: the plain launch's output; only: the partial sums, read and left as they were
    assert torch.equal(y, partial if only else full)


def test_dp_down2_without_a_residual(dp_case):
    b, cin, cout, vol = 1, 8, 8, (4, 8, 128)
    d, h, w = vol
    x, packed, scale, shift, _, _, _ = dp_case(b, cin, cout, vol, 0, True)
    full = kernels.conv3d_bnrelu_wino(x, packed, cout, scale, shift, True)
    want = kernels.resample_trilinear(full, (d // 2, h // 2, w // 2))
    y = torch.empty_like(full)
    down = torch.empty_like(want)
    kernels.conv3d_bnrelu_wino_dp_down2(x, packed, cout, scale, shift, True, y, down)
    assert torch.equal(y, full) and torch.equal(down, want)
    down.fill_(7.0)
    kernels.conv3d_bnrelu_wino_dp_down2(x, packed, cout, scale, shift, True, None, down, only=True)
    assert torch.equal(down, want)


def test_dp_down2_refuses_what_the_tiles_do_not_take():
    lib = _lib.load()
    x = torch.zeros(1, 8, 4, 4, 64, device=DEV)
    assert kernels.conv3d_wino_dp_down2_supported(x, 8)
    assert not kernels.conv3d_wino_dp_down2_supported(x.cpu(), 8)
    assert not kernels.conv3d_wino_dp_down2_supported(x.to(torch.bfloat16), 8)
    wp = torch.zeros(lib.lea_conv3d_wino_packed_floats(16, 8), device=DEV)
    for cout, vol in [(8, (3, 4, 64)),    # odd D
                      (8, (4, 5, 64)),    # odd H
                      (8, (4, 4, 66)),    # W % 4 != 0
                      (16, (4, 4, 64))]:  # cout > 8: not a depth-paired tile
        d, h, w = vol
        xs = torch.zeros((1, 8) + vol, device=DEV)
        assert not kernels.conv3d_wino_dp_down2_supported(xs, cout), (cout, vol)
        assert kernels.wino_dp_down2_kernel_name(1, 8, cout, d, h, w) is None
        y = torch.full((1, cout) + vol, 7.0, device=DEV)
        y2 = torch.full((1, cout, max(d // 2, 1), max(h // 2, 1), max(w // 2, 1)), 7.0, device=DEV)
        for yp in (y.data_ptr(), None):  # side, only
            rc = lib.lea_conv3d_bnrelu_wino_dp_down2(xs.data_ptr(), xs.stride(0), wp.data_ptr(), None, None,
                                                     y.data_ptr(), y.stride(0), yp, y.stride(0), y2.data_ptr(),
                                                     y2.stride(0), 1, 8, cout, d, h, w, _lib.LEA_RESIDUAL,
                                                     _lib.LEA_F32, None)
            assert rc == 1002, (cout, vol, rc)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()) and bool((y2 == 7.0).all())  # nothing launched


# ------------------------------------------------- s1's level-down copy: the up-sampling's side output
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("b,c,vol", [
    (1, 8, (2, 2, 8)),      # one plane pair per source pair, every window clamps at the far edge
    (2, 8, (3, 5, 12)),     # odd source sizes, batch strides
    (1, 3, (8, 6, 40))])    # three channels, more rows than one workgroup's 16
def test_resample_down2_is_bit_identical(b, c, vol, affine):
    g = torch.Generator().manual_seed(c + sum(vol))
    z = torch.randn((b, c + 2) + vol, generator=g).to(DEV)[:, 1:c + 1]   # a channel slice
    up = tuple(2 * n for n in vol)
    scale = (torch.rand(c, generator=g) + 0.5).to(DEV) if affine else None
    shift = (torch.randn(c, generator=g) * 0.3).to(DEV) if affine else None
    assert kernels.resample_down2_supported(z, up)
    mid = kernels.resample_trilinear(z, up, True, None, scale, shift, affine)
    if affine:
        assert float((mid == 0).float().mean()) > 0.05
    want = kernels.resample_trilinear(mid, vol)
    out = torch.full((b, c + 1) + up, 7.0, device=DEV)
    down = torch.full((b, c + 1) + vol, 7.0, device=DEV)
    with kernels.KernelProbe() as probe:
        kernels.resample_trilinear_down2(z, up, out[:, :c], down[:, 1:], scale, shift, affine)
    assert [r[0] for r in probe.records] == ["resample3d_sep_down2_f32"]
    assert torch.equal(out[:, :c], mid) and torch.equal(down[:, 1:], want)
    assert bool((out[:, c:] == 7.0).all()) and bool((down[:, :1] == 7.0).all())  # nothing past the slices


def test_resample_down2_other_ratios_and_refusals():
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    z = torch.randn((1, 2, 3, 5, 7), generator=g).to(DEV)
    for up in [(4, 8, 12), (6, 4, 8), (4, 10, 16), (4, 40, 12)]:  # not twice; H down; several row groups
        assert kernels.resample_down2_supported(z, up)
        mid = kernels.resample_trilinear(z, up)
        y, y2 = kernels.resample_trilinear_down2(z, up)
        assert torch.equal(y, mid) and torch.equal(y2, kernels.resample_trilinear(mid, tuple(n // 2 for n in up))), up
    assert not kernels.resample_down2_supported(z, (2, 10, 16))    # down-sampling along D
    assert not kernels.resample_down2_supported(z, (6, 9, 16))     # odd H
    assert not kernels.resample_down2_supported(z, (6, 10, 14))    # W % 4 != 0
    assert not kernels.resample_down2_supported(z.cpu(), (6, 10, 16))
    y = torch.full((1, 2, 6, 9, 16), 7.0, device=DEV)
    y2 = torch.full((1, 2, 3, 4, 8), 7.0, device=DEV)
    rc = lib.lea_resample3d_trilinear_down2(z.data_ptr(), z.stride(0), y.data_ptr(), y.stride(0), y2.data_ptr(),
                                            y2.stride(0), 1, 2, 3, 5, 7, 6, 9, 16, None, None, 0, _lib.LEA_F32, None)
    assert rc == 1002, rc
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((y2 == 7.0).all())


# ---------------------------------------------------------------------- whole model
@pytest.fixture(scope="module")
def model():
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=48)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def _forward(m, left, right, cells):
    old = executor.MatchingExecutor.FUSED_DOWN_CELLS
    executor.MatchingExecutor.FUSED_DOWN_CELLS = cells
    try:
        with torch.no_grad(), kernels.KernelProbe() as probe:
            disp = m(left, right)
        return disp, [(r[0], r[6]) for r in probe.records]
    finally:
        executor.MatchingExecutor.FUSED_DOWN_CELLS = old


def _routes(height, width, maxdisp, b=1):
    """(conv1's route, cell 10's route) at an input size, from the library's own queries: the
    planner's tile for conv1 (64 + 64 -> 64 at L1) and for cell 10's 8 -> 8 ops (L0), which run
    the Winograd engine only above its volume threshold."""
    lib = _lib.load()
    l0 = (maxdisp // 3, height // 3, width // 3)
    l1 = tuple(n // 2 for n in l0)
    conv1 = bool(kernels.wino_preferred(b, 64, 128, *l1) and lib.lea_conv3d_wino_down2_cat_supported(b, 128, 64, 64, *l1))
    cell10 = bool(kernels.wino_preferred(b, 8, 8, *l0) and lib.lea_conv3d_wino_dp_down2_supported(b, 8, 8, *l0)
                  and kernels.resample_down2_shape_supported(l1, l0))
    return conv1, cell10


def _is_resampling_conv(name):
    return name.startswith("conv1x1_rs") or (name.startswith("conv3d_reg_kernel") and name.endswith("true>"))


def _check_routes(recs_on, recs_off, conv1, cell10):
    """What FUSED_DOWN_CELLS changes in the launch list.  conv1's route: its launch becomes the
    two-input DOWN form and cells.5.share (64 -> 64) leaves the resampling gather-GEMM for a plain
    1x1.  Cell 10's route: s1's up-sampling writes the level-down copy too, the three launches
    that finish its steps become DOWN forms (the last one `only`) and cell 11's preprocess
    (32 -> 16) a plain 1x1.  Launch for launch, and no other resampling conv goes away."""
    on, off = [n for n, _ in recs_on], [n for n, _ in recs_off]
    new = ("conv3d_wino44_down2_cat_kernel", "conv3d_wino_dp_down2_kernel", "resample3d_sep_down2_f32")
    assert not [n for n in off if n.startswith(new)]
    assert on.count("conv3d_wino44_down2_cat_kernel") == int(conv1)
    assert on.count("resample3d_sep_down2_f32") == int(cell10)
    dp = [n for n in on if n.startswith("conv3d_wino_dp_down2_kernel")]
    assert len(dp) == 3 * int(cell10) and [n.endswith("true>") for n in dp] == [False, False, True][:len(dp)]
    assert len(on) == len(off)
    assert off.count("resample3d_f32") == on.count("resample3d_f32") + int(cell10)
    rs_on = Counter((n, s[1:3]) for n, s in recs_on if _is_resampling_conv(n))
    rs_off = Counter((n, s[1:3]) for n, s in recs_off if _is_resampling_conv(n))
    gone = sorted(cio for _, cio in (rs_off - rs_on).elements())
    assert not (rs_on - rs_off) and gone == sorted([(64, 64)] * int(conv1) + [(32, 16)] * int(cell10)), (rs_on, rs_off)
    if conv1:
        assert off.count("conv3d_wino44_kernel") == on.count("conv3d_wino44_kernel") + 1


def test_cells_route_runs_and_meets_the_e2e_bar(model):
    c = meta()["cases"]["e2e/b1_h96_w192_md48"]
    shape = (1, 3, c["height"], c["width"])
    left, right = normal(c["seeds"][0], shape).to(DEV), normal(c["seeds"][1], shape).to(DEV)
    on, recs = _forward(model, left, right, True)
    off, recs0 = _forward(model, left, right, False)
    conv1, cell10 = _routes(c["height"], c["width"], 48)
    print(f"routes at the golden shape: conv1 {conv1}, cell 10 {cell10}")
    # the golden case's L0 volume (16 x 32 x 64) is below the Winograd engine's threshold for the
    # 8-channel ops: cell 10's route is not taken there (test_cell10_route_at_a_larger_shape covers it)
    assert conv1 and not cell10 and not kernels.wino_preferred(1, 8, 8, 16, 32, 64)
    _check_routes(recs, recs0, conv1, cell10)
    g = golden("e2e")
    e32 = ref.epe(on.cpu(), torch.from_numpy(g["b1_h96_w192_md48/disp32"]))
    e64 = ref.epe(on.cpu(), torch.from_numpy(g["b1_h96_w192_md48/disp64"]))
    diff = ref.epe(on.cpu(), off.cpu())
    print(f"on vs golden: EPE {e32:.3e} (f32) {e64:.3e} (f64) px; on vs off: EPE {diff:.3e} px, "
          f"max {float((on - off).abs().max()):.3e} px")
    assert e32 < E2E_BAR and e64 < E2E_BAR, (e32, e64)
    assert diff < E2E_BAR, diff


def test_cells_route_batch_rows_are_independent(model):
    left = normal(911, (2, 3, 96, 192)).to(DEV)
    right = normal(912, (2, 3, 96, 192)).to(DEV)
    both, recs = _forward(model, left, right, True)
    assert "conv3d_wino44_down2_cat_kernel" in [n for n, _ in recs]
    one = torch.cat([_forward(model, left[i:i + 1], right[i:i + 1], True)[0] for i in range(2)])
    assert torch.equal(both, one)
    plain, _ = _forward(model, left, right, False)
    for i in range(2):
        assert ref.epe(both[i].cpu(), plain[i].cpu()) < E2E_BAR


def test_cell10_route_at_a_larger_shape(model):
    """288 x 576, D 48: an L0 volume (16 x 96 x 192) above the engine's threshold with whole
    64-wide tile rows -- cell 10's route on its 64-wide depth-paired tile, two batch rows.  (Every
    volume threshold of the engine choice falls on the same side for one and for two rows here,
    so a row's bits do not depend on the batch.)"""
    height, width = 288, 576
    conv1, cell10 = _routes(height, width, 48, b=2)
    assert cell10 and _routes(height, width, 48) == (conv1, cell10)
    left = normal(921, (2, 3, height, width)).to(DEV)
    right = normal(922, (2, 3, height, width)).to(DEV)
    on, recs = _forward(model, left, right, True)
    off, recs0 = _forward(model, left, right, False)
    _check_routes(recs, recs0, conv1, cell10)
    assert "conv3d_wino_dp_down2_kernel<16, true>" in [n for n, _ in recs]
    diff = ref.epe(on.cpu(), off.cpu())
    print(f"288 x 576: on vs off EPE {diff:.3e} px, max {float((on - off).abs().max()):.3e} px")
    assert diff < E2E_BAR, diff
    one, _ = _forward(model, left[1:], right[1:], True)
    assert torch.equal(on[1:], one)
