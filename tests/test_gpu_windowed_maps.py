"""stem0's 2D maps on the columns the f32 combine kernels read (lea_conv2d_bnrelu_windowed,
lea_cv_stem_map_windows, LEA_CVS_TMAJOR): the masked left maps on [0, D3 + 4), the K2 maps on
column 0 and [W - D3, W), the others on every column.  The route skips work and changes no
arithmetic, so every comparison is torch.equal: the map buffers start as NaN, the windowed
launches fill them, and lea_cv_stem_combine / lea_cv_stem_combine_down2 on them equal the same
calls on the full maps; outside the windows (rounded outward to the 16-column tiles) the buffers
are still NaN.

Shapes (C = 4 feature channels): D3 = 8 at W = 64 (both windows and an unwritten interior),
W = 36 (not a multiple of the tile), W = 20 (the windows merge and cover everything), D3 = 64 at
W = 64 (D3 >= W: everything is in the band), batch 2."""
import pytest
import torch

from leastereo_amd import _lib, kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 4

# (batch, cout, maxdisp, H, W)
SHAPES = [(1, 8, 24, 6, 64), (1, 16, 24, 8, 64), (1, 8, 24, 6, 36), (1, 16, 24, 8, 36), (1, 8, 24, 8, 20),
          (1, 16, 192, 6, 64), (2, 8, 24, 8, 64), (2, 16, 24, 6, 36)]


def _columns(w, tiles):
    """bool [W]: the columns inside the windows as run (16-column tiles)."""
    m = torch.zeros(w, dtype=torch.bool)
    for s, e in tiles:
        m[16 * s:16 * e] = True
    return m.to(DEV)


@pytest.fixture(scope="module")
def case():
    memo = {}

    def get(b, cout, maxdisp, h, w):
        key = (b, cout, maxdisp, h, w)
        if key not in memo:
            d3 = maxdisp // 3
            g = torch.Generator(device=DEV).manual_seed(cout + maxdisp + h + w)
            fl = torch.randn((b, C, 1, h, w), device=DEV, generator=g)
            fr = torch.randn((b, C, 1, h, w), device=DEV, generator=g)
            wt = torch.randn((cout, 2 * C, 3, 3, 3), device=DEV, generator=g) / (54 * C) ** 0.5
            scale = torch.rand(cout, device=DEV, generator=g) + 0.5
            shift = torch.randn(cout, device=DEV, generator=g) * 0.3  # some outputs negative: the ReLU matters
            wl, wr = kernels.cv_stem_split_weights(wt)
            lm = kernels.conv2d_bnrelu(fl, kernels.pack_conv2d_weight(wl), 9 * cout, None, None, relu=False)
            rm = kernels.conv2d_bnrelu(fr, kernels.pack_conv2d_weight(wr), 6 * cout, None, None, relu=False)
            # the windowed route's maps: left rows (3 kd + t) cout + o -> t-major
            wlt = wl.view(3, 3, cout, C, 3, 3).transpose(0, 1).reshape(wl.shape)
            lwin, rwin = kernels.cv_stem_map_windows(d3, w)
            lmw = torch.full_like(lm, float("nan"))
            rmw = torch.full_like(rm, float("nan"))
            kernels.conv2d_bnrelu_windowed(fl, kernels.pack_conv2d_weight_windowed(wlt, 3 * cout), 9 * cout, 3 * cout,
                                           (lwin,), out=lmw)
            kernels.conv2d_bnrelu_windowed(fr, kernels.pack_conv2d_weight_windowed(wr, 3 * cout), 6 * cout, 3 * cout,
                                           rwin, out=rmw)
            memo[key] = (d3, scale, shift, lm, rm, lmw, rmw, lwin, rwin)
        return memo[key]
    return get


def test_windows_are_the_kernels_conditions():
    assert kernels.cv_stem_map_windows(8, 64) == ((0, 12), ((0, 1), (56, 64)))
    assert kernels.cv_stem_map_windows(64, 320) == ((0, 68), ((0, 1), (256, 320)))
    assert kernels.cv_stem_map_windows(64, 64) == ((0, 64), ((0, 1), (1, 64)))
    assert kernels.cv_stem_map_windows(64, 20) == ((0, 20), ((0, 1), (1, 20)))
    # as run: rounded outward to the tiles, one window where they touch
    assert kernels.conv2d_windowed_tiles(64, [(0, 12)]) == [(0, 1)]
    assert kernels.conv2d_windowed_tiles(64, [(0, 1), (56, 64)]) == [(0, 1), (3, 4)]
    assert kernels.conv2d_windowed_tiles(36, [(0, 1), (28, 36)]) == [(0, 3)]
    assert kernels.conv2d_windowed_tiles(20, [(0, 1), (12, 20)]) == [(0, 2)]
    assert kernels.conv2d_windowed_tiles(320, [(0, 1), (256, 320)]) == [(0, 1), (16, 20)]
    lib = _lib.load()
    import ctypes
    t = (ctypes.c_int * 4)()
    assert lib.lea_conv2d_windowed_tiles(64, 8, 4, 0, 0, t) == 1001     # an empty first window
    assert lib.lea_conv2d_windowed_tiles(64, 0, 32, 16, 64, t) == 1001  # overlapping windows
    assert lib.lea_conv2d_windowed_tiles(64, 0, 8, 32, 65, t) == 1001   # past the last column


@pytest.mark.parametrize("b,cout,maxdisp,h,w", SHAPES)
def test_nothing_is_written_outside_the_windows(case, b, cout, maxdisp, h, w):
    d3, _, _, lm, rm, lmw, rmw, lwin, rwin = case(b, cout, maxdisp, h, w)
    for full, win, windows, tmajor in ((lm, lmw, [lwin], True), (rm, rmw, list(rwin), False)):
        inside = _columns(w, kernels.conv2d_windowed_tiles(w, windows))
        assert not win[:, :3 * cout].isnan().any()
        assert not win[:, 3 * cout:][..., inside].isnan().any()
        assert win[:, 3 * cout:][..., ~inside].isnan().all()
        # where computed, a map is the full launch's map (left: channel (3 t + kd) cout + o of the
        # windowed buffer is channel (3 kd + t) cout + o of the public order)
        if tmajor:
            full = full.view(b, 3, 3, cout, 1, h, w).transpose(1, 2).reshape(full.shape)
        assert torch.equal(win[:, :3 * cout], full[:, :3 * cout])
        assert torch.equal(win[:, 3 * cout:][..., inside], full[:, 3 * cout:][..., inside])
    if (maxdisp, w) == (24, 64):  # both windows and an interior that no workgroup touched
        assert int((~_columns(w, kernels.conv2d_windowed_tiles(w, list(rwin)))).sum()) == 32
        assert int((~_columns(w, kernels.conv2d_windowed_tiles(w, [lwin]))).sum()) == 48


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("b,cout,maxdisp,h,w", SHAPES)
def test_combine_on_windowed_maps_is_combine_on_full_maps(case, b, cout, maxdisp, h, w, relu):
    d3, scale, shift, lm, rm, lmw, rmw, _, _ = case(b, cout, maxdisp, h, w)
    want = kernels.cv_stem_combine(lm, rm, cout, d3, scale, shift, relu)
    got = kernels.cv_stem_combine(lmw, rmw, cout, d3, scale, shift, relu, tmajor=True)
    assert not want.isnan().any()
    assert torch.equal(got, want)
    if relu:
        assert float((want == 0).float().mean()) > 0.05
    assert kernels.cv_stem_down2_supported(lm, cout, d3) == (d3 % 2 == 0 and h % 2 == 0 and w % 4 == 0)
    if kernels.cv_stem_down2_supported(lm, cout, d3):
        want, want2 = kernels.cv_stem_combine_down2(lm, rm, cout, d3, scale, shift, relu)
        got, got2 = kernels.cv_stem_combine_down2(lmw, rmw, cout, d3, scale, shift, relu, tmajor=True)
        assert not want2.isnan().any()
        assert torch.equal(got, want) and torch.equal(got2, want2)


def test_the_flag_is_f32_only_and_the_entry_refuses_a_residual():
    lib = _lib.load()
    x = torch.zeros(1, 8, 1, 4, 16, device=DEV)
    y = torch.zeros(1, 16, 1, 4, 16, device=DEV)
    p = lambda t: t.data_ptr()
    assert lib.lea_conv2d_bnrelu_windowed(p(x), x.stride(0), p(x), None, None, p(y), y.stride(0), 1, 8, 16, 8, 4, 16,
                                          0, 8, 0, 0, _lib.LEA_RESIDUAL, _lib.LEA_F32, None) == 1001
    assert lib.lea_conv2d_bnrelu_windowed(p(x), x.stride(0), p(x), None, None, p(y), y.stride(0), 1, 8, 16, 16, 4, 16,
                                          0, 8, 0, 0, 0, _lib.LEA_F32, None) == 1001   # split == cout
    assert lib.lea_cv_stem_combine(p(x), 0, p(x), 0, None, None, p(y), 0, 1, 8, 4, 4, 16, _lib.LEA_CVS_TMAJOR,
                                   _lib.LEA_BF16, None) == 1001
    assert b"f32 only" in lib.lea_last_error()
