"""GPU checks of what the tensor wrappers (leastereo_amd/kernels.py) share among themselves: the
probe records of the launch helper, and the null-safe pointer and exclude-mask helpers on the
wrappers that take optional outputs.

Probe records: the expected ``flops``, ``bytes``, ``mfma_flops`` and ``shape`` are written out
here as arithmetic on the layer shape (the accounting rules of ``KernelProbe``: direct-conv
FLOPs, the bytes the launch really moves, the matrix-core products of the tile that runs) and
compared with ``==``.  The shapes are one small volume that the ``*_supported`` queries accept
for the depth-paired tile (8 channels) and for the F(4,3) x F(4,3) tile (32 channels)."""
import pytest
import torch

from leastereo_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
VOL = (4, 8, 16)


def _layer(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, cin) + VOL, generator=g).to(DEV)
    wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5).to(DEV)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(cout, generator=g) * 0.3).to(DEV)
    return x, kernels.pack_conv_weight_wino(wt), scale, shift


def _one_record(probe, name):
    assert [r.name for r in probe.records] == [name]
    r = probe.records[0]
    assert isinstance(r, tuple) and len(r) == 7 and r[0] == r.name and r[2] == r.bytes and r[6] == r.shape
    assert set(probe.summary()) == {name} and set(probe.by_shape(name)) == {r.shape}
    assert probe.summary()[name]["bytes"] == r.bytes and probe.by_shape(name)[r.shape]["flops"] == r.flops
    return r


def _mfma_scale(cout, plain_name):
    """Matrix-core products per direct-conv product of the tile ``plain_name`` names."""
    if plain_name == "conv3d_wino44_kernel":  # F(4,3) x F(4,3), couts padded to 32
        return (-(-cout // 32) * 32) / cout / 4.0
    assert plain_name.startswith("conv3d_wino_kernel<") and cout <= 8, plain_name  # depth-paired F(f,3) along W
    f = int(plain_name.split("<", 1)[1].split(",", 1)[0])
    return (f + 2) / (3.0 * f) * 12 / 9 * 8 / cout


@pytest.mark.parametrize("c", [8, 32])
def test_probe_record_of_the_plain_winograd_conv(c):
    b, cin, cout, (d, h, w) = 1, c, c, VOL
    x, packed, scale, shift = _layer(cin, cout, 11 + c)
    name = kernels.wino_kernel_name(b, cout, d, h, w, cin=cin)
    with kernels.KernelProbe() as probe:
        kernels.conv3d_bnrelu_wino(x, packed, cout, scale, shift, True)
    r = _one_record(probe, name)
    vox = b * d * h * w
    flops = 2.0 * vox * cout * cin * 3 ** 3
    assert r.flops == flops
    assert r.bytes == 4 * (vox * cin + vox * cout * 1) + 4.0 * cout * cin * 3 ** 3
    assert r.mfma_flops == flops * _mfma_scale(cout, name)
    assert r.shape == (b, cin, cout, d, h, w, 3)


def test_probe_record_of_wino_down2_overrides_the_bytes():
    b, cin, cout, (d, h, w) = 1, 32, 32, VOL
    x, packed, scale, shift = _layer(cin, cout, 21)
    assert kernels.conv3d_wino_down2_supported(x, cout)
    with kernels.KernelProbe() as probe:
        got = kernels.conv3d_bnrelu_wino_down2(x, packed, cout, scale, shift, True)
    r = _one_record(probe, "conv3d_wino44_down2_kernel")
    flops = 2.0 * (b * d * h * w) * cout * cin * 3 ** 3
    assert r.flops == flops
    # the bytes really moved: input + weights + the half-size output (the full one is never written)
    assert r.bytes == 4.0 * (b * cin * d * h * w + got.numel()) + 4.0 * cout * cin * 27
    assert r.mfma_flops == flops * _mfma_scale(cout, "conv3d_wino44_kernel")
    assert r.shape == (b, cin, cout, d, h, w, 3)
    assert got.shape == (b, cout, d // 2, h // 2, w // 2)


@pytest.mark.parametrize("only,accumulate", [(False, False), (True, False), (True, True)],
                         ids=["side", "only", "only-accumulate"])
def test_probe_record_of_wino_dp_down2_overrides_the_bytes(only, accumulate):
    b, cin, cout, (d, h, w) = 1, 8, 8, VOL
    x, packed, scale, shift = _layer(cin, cout, 31)
    assert kernels.conv3d_wino_dp_down2_supported(x, cout)
    out = None if (only and not accumulate) else torch.zeros((b, cout) + VOL, device=DEV)
    down = torch.empty((b, cout, d // 2, h // 2, w // 2), device=DEV)
    with kernels.KernelProbe() as probe:
        got = kernels.conv3d_bnrelu_wino_dp_down2(x, packed, cout, scale, shift, True, out, down,
                                                  accumulate=accumulate, only=only)
    assert got is down
    r = _one_record(probe, f"conv3d_wino_dp_down2_kernel<8, {'true' if only else 'false'}>")
    flops = 2.0 * (b * d * h * w) * cout * cin * 3 ** 3
    assert r.flops == flops
    # the bytes really moved: input, weights, the residual read, the full output unless `only`, the half one
    vox = b * cout * d * h * w
    assert r.bytes == 4.0 * (x.numel() + (vox if accumulate else 0) + (0 if only else vox) + down.numel()) \
        + 4.0 * cout * cin * 27
    assert r.mfma_flops == flops * _mfma_scale(cout, kernels.wino_kernel_name(b, cout, d, h, w, cin=cin))
    assert r.shape == (b, cin, cout, d, h, w, 3)


def test_a_name_filter_records_only_its_kernels_and_no_probe_records_nothing():
    x, packed, scale, shift = _layer(32, 32, 41)
    with kernels.KernelProbe(names=["conv3d_wino44_down2_kernel"]) as probe:
        kernels.conv3d_bnrelu_wino(x, packed, 32, scale, shift, True)
        kernels.conv3d_bnrelu_wino_down2(x, packed, 32, scale, shift, True)
    assert [r.name for r in probe.records] == ["conv3d_wino44_down2_kernel"]
    kernels.conv3d_bnrelu_wino(x, packed, 32, scale, shift, True)
    assert len(probe.records) == 1 and kernels._probe is None


# ------------------------------------------------- optional outputs and the exclude mask
H, W = 8, 16


def _disp(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((1, H, W), generator=g) * 6.0 + 1.0).to(DEV)


def _mask(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((1, H, W), generator=g) < 0.25).to(DEV)


def test_speckle_filter_null_outputs_and_bool_exclude():
    disp = _disp(51)
    r = kernels.speckle_filter(disp, exclude=None, want_labels=False, want_size=False, want_filtered=False)
    assert r.size is None and r.labels is None and r.filtered is None
    assert r.disp is disp and r.state.dtype == torch.uint8 and tuple(r.state.shape) == (1, H, W)
    ex = _mask(52)
    rb = kernels.speckle_filter(disp, exclude=ex, want_labels=True)
    ru = kernels.speckle_filter(disp, exclude=ex.to(torch.uint8), want_labels=True)
    for got, want in zip(rb[1:], ru[1:]):
        assert torch.equal(got, want)
    assert bool((rb.state[ex] == 1).all()) and bool((rb.labels[ex] == -1).all())


def test_reproject_null_outputs_and_bool_exclude():
    disp = _disp(61)
    q = torch.eye(4)
    r = kernels.reproject(disp, q, want_points=False, want_valid=True, want_compact=False)
    assert all(t is None for t in (r.points, r.count, r.xyz, r.rgb, r.index, r.normals))
    assert r.valid.dtype == torch.uint8 and tuple(r.valid.shape) == (1, H, W)
    ex = _mask(62)
    rb = kernels.reproject(disp, q, exclude=ex, want_valid=True)
    ru = kernels.reproject(disp, q, exclude=ex.to(torch.uint8), want_valid=True)
    assert rb.points is None and rb.rgb is None and rb.normals is None
    assert torch.equal(rb.valid, ru.valid) and torch.equal(rb.count, ru.count)
    assert bool((rb.valid[ex] == 0).all())
    n = int(rb.count[0])
    assert n == int(rb.valid.sum()) and torch.equal(rb.xyz[0, :n], ru.xyz[0, :n])
    assert torch.equal(rb.index[0, :n], ru.index[0, :n])


def test_forward_warp_null_outputs_and_bool_exclude():
    disp = _disp(71)
    g = torch.Generator().manual_seed(72)
    image = torch.rand((1, 3, H, W), generator=g).to(DEV)
    r = kernels.forward_warp(image, disp, exclude=None, want_zview=False, want_state=False, want_source=False)
    assert r.zview is None and r.state is None and r.source is None
    assert tuple(r.image.shape) == (1, 3, H, W) and r.image.dtype == torch.float32
    ex = _mask(73)
    rb = kernels.forward_warp(image, disp, exclude=ex, want_zview=False, want_source=False)
    ru = kernels.forward_warp(image, disp, exclude=ex.to(torch.uint8), want_zview=False, want_source=False)
    assert rb.zview is None and rb.source is None
    assert rb.state.dtype == torch.uint8 and tuple(rb.state.shape) == (1, H, W)
    assert torch.equal(rb.state, ru.state) and torch.equal(rb.image, ru.image)
    assert not torch.equal(rb.image, r.image)  # the mask took effect
