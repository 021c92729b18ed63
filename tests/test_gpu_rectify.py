"""Rectification on the GPU (lea_rectify_pair_u8, kernels.rectify_u8, rectify.Rectifier,
predict.py --calib) against tests/rectify_judge.py.

A lane owns four consecutive pixels of an output row; a workgroup 128 x 8 pixels (or 1024 x 1
under lea_rectify_set_tile(1)).  The lane's bytes are stored as dwords where their address is
4-byte aligned, else with a byte head and tail, so the shapes pin odd widths at both pixel
strides, rows shorter than a lane's four pixels, more than one workgroup along each axis and
several images.  Every output is written into a buffer filled with a sentinel, with 256 guard
elements either side.

  * pixel stage (maps given): images, valid and the fill pattern equal the judge bit for bit, no
    pixel left out;
  * map stage (calibration given): the largest error of the maps against the float64 judge is
    at most max(4 x the float32 restatement's largest error in that case, 8 ulp of the case's
    largest |coordinate|), the standing bar of the float heads, and the NaN pattern is the
    judge's.
"""
import functools

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels
from leastereo_amd import rectify as rc
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from tests import rectify_judge as rj
from tests.golden_util import golden, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT, SENT_BYTE, GUARD = 0x7FC0DEAD, 0xAB, 256
IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def run_raw(left, right, calib=None, maps=None, size=None, fill=0):
    """The C entry with every output asked for, in sentinel-filled buffers with guard bands:
    dict(left, right, valid, maps) as numpy."""
    B, H, W, ps = left.shape
    Ho, Wo = size if maps is None else maps.shape[-2:]
    lib = _lib.load()
    dl, dr, dc, dm = _dev(left), _dev(right), _dev(calib), _dev(maps)
    n = B * Ho * Wo
    sizes = dict(left=(n * ps, torch.uint8), right=(n * ps, torch.uint8), valid=(2 * n, torch.uint8),
                 maps=(4 * n, torch.int32))
    bufs = {k: torch.full((m + 2 * GUARD,), SENT if t == torch.int32 else SENT_BYTE, device=DEV, dtype=t)
            for k, (m, t) in sizes.items()}
    p = {k: v.data_ptr() + GUARD * v.element_size() for k, v in bufs.items()}
    kernels.check(lib.lea_rectify_pair_u8(
        dl.data_ptr(), dr.data_ptr(), ps, B, H, W, None if dc is None else dc.data_ptr(),
        0 if dc is None else dc.shape[0], None if dm is None else dm.data_ptr(), 0 if dm is None else dm.shape[0],
        Ho, Wo, fill, p["left"], p["right"], p["valid"], p["maps"], None), "rectify")
    torch.cuda.synchronize()
    out = {}
    for k, v in bufs.items():
        a = v.cpu().numpy()
        s = SENT if a.dtype == np.int32 else SENT_BYTE
        assert (a[:GUARD] == s).all() and (a[-GUARD:] == s).all(), f"{k}: a guard band was written"
        out[k] = a[GUARD:-GUARD]
    assert np.array_equal(dl.cpu().numpy(), left) and np.array_equal(dr.cpu().numpy(), right)  # the inputs too
    out["left"], out["right"] = out["left"].reshape(B, Ho, Wo, ps), out["right"].reshape(B, Ho, Wo, ps)
    out["valid"] = out["valid"].reshape(B, 2, Ho, Wo)
    out["maps"] = out["maps"].view(np.float32).reshape(B, 2, 2, Ho, Wo)
    return out


def assert_pixels_are_judge(out, left, right, maps, fill, what):
    jl, jr, jv = rj.rectify_judge(left, right, maps, fill)
    assert np.array_equal(out["valid"], jv), what
    assert np.array_equal(out["left"], jl), (what, int((out["left"] != jl).sum()))
    assert np.array_equal(out["right"], jr), (what, int((out["right"] != jr).sum()))
    return jv


# (B, Ho, Wo) of the issue, then an output wider and taller than its source
OUT_SHAPES = [(1, 1, 1), (1, 1, 257), (1, 33, 1), (2, 67, 131), (1, 5, 3), (1, 7, 5), (3, 40, 50), (1, 140, 300)]
SOURCES = [(61, 127), (1, 1), (2, 2)]


@pytest.mark.parametrize("ps", [3, 4])
@pytest.mark.parametrize("shape", OUT_SHAPES, **IDS)
def test_pixel_stage_is_the_judge_bit_for_bit(shape, ps):
    B, Ho, Wo = shape
    i = OUT_SHAPES.index(shape)
    sources = SOURCES if shape in ((2, 67, 131), (3, 40, 50)) else [SOURCES[(i + ps) % 3]]
    if shape == (1, 140, 300):
        sources = [(61, 127)]
    for H, W in sources:
        img = rj.recipe_image((2 * B, H, W), ps, seed=7 + i)
        left, right = img[:B], img[B:]
        for Bm in sorted({1, B}):
            fill = 171 if (i + Bm + ps) % 2 else 0
            maps = rj.plant_specials(rj.smooth_warp(Bm, Ho, Wo, H, W, seed=3 + i + Bm), H, W, seed=11 + i)
            out = run_raw(left, right, maps=maps, fill=fill)
            assert np.array_equal(out["maps"].view(np.int32), np.broadcast_to(maps, out["maps"].shape).view(np.int32))
            jv = assert_pixels_are_judge(out, left, right, maps, fill, (shape, ps, (H, W), Bm, fill))
            if Ho * Wo > 1000:
                assert 0.2 < jv.mean() < 0.9  # both kinds of pixel in numbers


def test_pixel_stage_every_special_value_on_every_source():
    """Each special coordinate against each other one, in x and y, on the three sources and a
    fill that is no image value of the recipe's neighbourhood."""
    for ps in (3, 4):
        for H, W in SOURCES:
            sx, sy = np.meshgrid(rj.special_values(W), rj.special_values(H))
            maps = np.ascontiguousarray(np.stack([np.stack([sx, sy]), np.stack([sx[:, ::-1], sy[::-1]])])[None])
            assert maps.dtype == np.float32
            img = rj.recipe_image((2, H, W), ps, seed=H + W)
            for fill in (0, 171):
                out = run_raw(img[:1], img[1:], maps=maps, fill=fill)
                jv = assert_pixels_are_judge(out, img[:1], img[1:], maps, fill, (ps, H, W, fill))
                assert 0 < jv.sum() < jv.size


@functools.lru_cache(maxsize=None)
def _rig_calib(name, out):
    cl, cr, R, T = rj.recipe_rig(name, (61, 127))
    return rc.stereo_rectify(cl, cr, R, T, (61, 127), out_size=out).calib()[0]


def map_bar(m32, m64):
    """max(4 x the float32 restatement's largest error, 8 ulp of the largest |coordinate|)."""
    ok = np.isfinite(m64)
    e32 = np.abs(m32.astype(np.float64) - m64)[ok].max()
    top = np.float32(np.abs(m64[ok]).max())
    return max(4 * e32, 8 * float(np.spacing(top))), e32


@pytest.mark.parametrize("out", [(67, 131), (130, 70)], **IDS)
@pytest.mark.parametrize("name", rj.RIGS)
def test_map_stage_against_the_float64_judge(name, out):
    Ho, Wo = out
    other = rj.RIGS[(rj.RIGS.index(name) + 1) % len(rj.RIGS)]
    img = rj.recipe_image((4, 61, 127), 3, seed=2)
    for calib in (_rig_calib(name, out)[None], np.stack([_rig_calib(name, out), _rig_calib(other, out)])):
        got = run_raw(img[:2], img[2:], calib=calib, size=out, fill=9)
        for b in range(2):
            c = calib[b if calib.shape[0] > 1 else 0]
            m64, m32 = rj.map64(c, Ho, Wo), rj.map32(c, Ho, Wo)
            g = got["maps"][b]
            assert np.array_equal(np.isnan(g), np.isnan(m64))
            bar, e32 = map_bar(m32, m64)
            err = np.abs(g.astype(np.float64) - m64)[np.isfinite(m64)].max()
            print(f"{name} {out} Bc={calib.shape[0]} b={b}: kernel {err:.3g} px, float32 judge {e32:.3g} px, "
                  f"bar {bar:.3g} px, ratio {err / bar:.3f}")
            assert err <= bar, (name, out, b, err, bar)
        # one copy of the arithmetic: the images are the pixel judge on the launch's own maps
        assert_pixels_are_judge(got, img[:2], img[2:], got["maps"], 9, (name, out, "own maps"))
        again = run_raw(img[:2], img[2:], maps=got["maps"], fill=9)
        for k in ("left", "right", "valid"):
            assert np.array_equal(again[k], got[k]), k
        assert np.array_equal(again["maps"].view(np.int32), got["maps"].view(np.int32))


def test_behind_the_camera_is_nan_and_fill():
    Ho, Wo = 67, 131
    c = rj.behind_calib(Ho, Wo)
    m64, wc = rj.map64(c, Ho, Wo, return_wc=True)
    assert np.abs(wc).min() > 1e-3                       # no pixel's side is a matter of rounding
    img = rj.recipe_image((2, 61, 127), 4, seed=4)
    got = run_raw(img[:1], img[1:], calib=c[None], size=(Ho, Wo), fill=171)
    assert np.array_equal(np.isnan(got["maps"][0]), np.isnan(m64)) and 0.05 < np.isnan(m64).mean() < 0.95
    assert_pixels_are_judge(got, img[:1], img[1:], got["maps"], 171, "behind")
    assert (got["valid"][0][np.isnan(m64[:, 0])] == 0).all()


def test_any_calibration_floats_are_memory_safe():
    """NaN, infinities, 1e30 and random bits as the 48 floats: the guards hold and the images are
    the pixel judge on the maps the launch reports."""
    rng = np.random.default_rng(8)
    img = rj.recipe_image((2, 61, 127), 3, seed=6)
    base = _rig_calib("rational8", (67, 131))
    cases = [np.full((2, 24), v, np.float32) for v in (np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0)]
    cases += [rng.integers(0, 2 ** 32, (2, 24), dtype=np.uint64).astype(np.uint32).view(np.float32) for _ in range(4)]
    for fld, v in ((8, 1e-30), (9, 1e30), (11, -1e30), (13, np.nan), (14, 1e30), (19, -1.0)):
        c = base.copy()
        c[:, fld] = v
        cases.append(c)
    for c in cases:
        got = run_raw(img[:1], img[1:], calib=c[None], size=(67, 131), fill=3)
        assert_pixels_are_judge(got, img[:1], img[1:], got["maps"], 3, "wild calibration")


@pytest.mark.parametrize("ps", [3, 4])
def test_exact_geometry_whole_pixel_shifts(ps):
    """fx = fy = 256, integer principal points, no distortion, R = I: a new camera matrix
    shifted by whole pixels gives the shifted source bit for bit, fill outside, valid exactly
    the overlap; unshifted it returns the input."""
    H, W = 61, 127
    img = rj.recipe_image((2, H, W), ps, seed=12)
    for (dx, dy), out in (((0, 0), (H, W)), ((5, -3), (H, W)), ((-17, 8), (70, 131)), ((200, 0), (H, W))):
        c = np.zeros((2, 24), np.float64)
        for k in range(2):
            Kn = np.array([[256.0, 0, 60 + dx], [0, 256.0, 30 + dy], [0, 0, 1]])
            c[k, :9] = np.linalg.inv(Kn).reshape(-1)
            c[k, 9:13] = 256.0, 256.0, 60.0, 30.0
        got = run_raw(img[:1], img[1:], calib=c.astype(np.float32)[None], size=out, fill=171)
        v, u = np.meshgrid(np.arange(out[0]), np.arange(out[1]), indexing="ij")
        sx, sy = u - dx, v - dy                               # the source pixel of an output pixel
        inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        assert np.array_equal(got["maps"][0, 0, 0], sx.astype(np.float32))
        assert np.array_equal(got["maps"][0, 1, 1], sy.astype(np.float32))
        for k, name in enumerate(("left", "right")):
            want = np.where(inside[..., None], img[k][np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], np.uint8(171))
            assert np.array_equal(got[name][0], want), (dx, dy, name)
            assert np.array_equal(got["valid"][0, k], inside.astype(np.uint8))
        if (dx, dy) == (0, 0):
            assert np.array_equal(got["left"][0], img[0]) and got["valid"].all()


def test_both_tiles_give_the_same_bits():
    lib = _lib.load()
    img = rj.recipe_image((4, 61, 127), 3, seed=2)
    c = np.stack([_rig_calib("rational8", (67, 131)), _rig_calib("fisheye", (67, 131))])
    a = run_raw(img[:2], img[2:], calib=c, size=(67, 131), fill=1)
    assert lib.lea_rectify_set_tile(2) == _lib.LEA_E_INVALID
    with _lib.tuning(lea_rectify_set_tile=1):
        b = run_raw(img[:2], img[2:], calib=c, size=(67, 131), fill=1)
        maps = rj.plant_specials(rj.smooth_warp(1, 33, 1031, 61, 127, seed=1), 61, 127, seed=5)
        wide = run_raw(img[:1], img[2:3], maps=maps, fill=171)   # two row-shaped workgroups along x
        assert_pixels_are_judge(wide, img[:1], img[2:3], maps, 171, "row tile")
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _rectification(name, out=(67, 131)):
    cl, cr, R, T = rj.recipe_rig(name, (61, 127))
    return rc.stereo_rectify(cl, cr, R, T, (61, 127), out_size=out)


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        assert x is None or torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_captured_rectifier_replays_with_a_new_calibration_and_new_images():
    img = rj.recipe_image((4, 61, 127), 4, seed=21)
    left, right = _dev(img[0]), _dev(img[1])
    r = rc.Rectifier(_rectification("pinhole5"), DEV, fill=17)
    _same(r(left, right, want_maps=True), r(left, right, want_maps=True))    # two eager calls
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r(left, right, want_maps=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = r(left, right, want_maps=True)
    graph.replay()
    _same(out, r(left, right, want_maps=True))
    first = out.maps.clone()
    r.update(_rectification("fisheye"))
    graph.replay()
    _same(out, r(left, right, want_maps=True))
    assert not torch.equal(first, out.maps)
    left.copy_(_dev(img[2])), right.copy_(_dev(img[3]))
    graph.replay()
    _same(out, r(left, right, want_maps=True))
    m = out.maps.cpu().numpy()
    jl, jr, jv = rj.rectify_judge(img[2:3], img[3:4], m[None], 17)
    assert np.array_equal(out.left.cpu().numpy(), jl[0]) and np.array_equal(out.valid.cpu().numpy(), jv[0])
    assert torch.equal(r.maps().view(torch.int32), out.maps.view(torch.int32))
    with pytest.raises(ValueError):
        r.update(_rectification("fisheye", out=(61, 127)))


def test_wrapper_shapes_and_refusals():
    img = rj.recipe_image((4, 61, 127), 3, seed=2)
    c = _rig_calib("toe_in", (67, 131))
    raw = run_raw(img[:2], img[2:], calib=c[None], size=(67, 131), fill=5)
    left, right = _dev(img[:2]), _dev(img[2:])
    out = kernels.rectify_u8(left, right, calib=c, size=(67, 131), fill=5, want_maps=True)
    assert isinstance(out, kernels.RectifiedPair) and out._fields == ("left", "right", "valid", "maps")
    for k in out._fields:
        assert np.array_equal(getattr(out, k).cpu().numpy().view(np.uint8), raw[k].view(np.uint8)), k
    one = kernels.rectify_u8(left[1], right[1], maps=out.maps[1], fill=5, want_valid=False)
    assert one.left.shape == (67, 131, 3) and one.valid is None and one.maps is None
    assert torch.equal(one.left, out.left[1]) and torch.equal(one.right, out.right[1])
    same = kernels.rectify_u8(left, right, calib=c)                       # default size: the input's
    assert same.left.shape == (2, 61, 127, 3) and same.valid.shape == (2, 2, 61, 127)
    with kernels.KernelProbe() as probe:
        kernels.rectify_u8(left, right, calib=c)
    assert probe.summary()["rectify_pair"]["launches"] == 1
    m = out.maps
    for kw in (dict(), dict(calib=c, maps=m), dict(calib=c, fill=256), dict(calib=c, fill=-1), dict(calib=c, fill=1.5),
               dict(calib=np.zeros((2, 23))), dict(calib=np.zeros((3, 2, 24))), dict(calib=c, size=(0, 5)),
               dict(maps=m[:, :1]), dict(maps=torch.zeros(3, 2, 2, 5, 5)), dict(maps=m, size=(5, 5)),
               dict(maps=m.to(torch.int32))):
        with pytest.raises(ValueError):
            kernels.rectify_u8(left, right, **kw)
    for l2, r2 in ((left.float(), right.float()), (left.cpu(), right.cpu()), (left, right[:, :60]),
                   (left[..., :2], right[..., :2]), (left[0, 0], right[0, 0])):
        with pytest.raises(ValueError):
            kernels.rectify_u8(l2, r2, calib=c)
    lib = _lib.load()
    t = torch.zeros(4096, device=DEV, dtype=torch.uint8)
    p = t.data_ptr()
    args = lambda **k: [k.get(n, d) for n, d in (  # noqa: E731
        ("left", p), ("right", p + 64), ("ps", 3), ("B", 1), ("H", 2), ("W", 2), ("calib", p + 256), ("Bc", 1),
        ("maps_in", None), ("Bm", 0), ("Ho", 2), ("Wo", 2), ("fill", 0), ("ol", p + 1024), ("or", p + 1100),
        ("valid", p + 1200), ("maps_out", p + 2048), ("stream", None))]
    for kw, word in ((dict(left=None), b"null"), (dict(ol=None), b"null"), (dict(ps=5), b"pix_stride"),
                     (dict(B=0), b"bad shape"), (dict(Wo=70000), b"65535"), (dict(maps_in=p + 512, Bm=1), b"exactly one"),
                     (dict(calib=None), b"exactly one"), (dict(Bc=2), b"calib batch"),
                     (dict(calib=None, maps_in=p + 512, Bm=3), b"maps_in batch"), (dict(fill=256), b"fill"),
                     (dict(fill=-1), b"fill"), (dict(ol=p), b"overlaps"), (dict(valid=p + 1024 + 11), b"overlaps"),
                     (dict(maps_out=p + 256), b"overlaps"), (dict(maps_out=p + 2050), b"aligned")):
        assert lib.lea_rectify_pair_u8(*args(**kw)) == _lib.LEA_E_INVALID, kw
        assert word in lib.lea_last_error() and b"lea_rectify_pair_u8" in lib.lea_last_error(), (kw, lib.lea_last_error())
    torch.cuda.synchronize()
    assert not t.any()


# ------------------------------------------------------------------ the chain
H, W, MD = 96, 192, 48


@functools.lru_cache(maxsize=None)
def _model():
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def _raw_rig(size):
    h, w = size
    Kl = [[0.9 * w, 0, 0.5 * w - 2], [0, 0.9 * w, 0.5 * h + 1], [0, 0, 1]]
    Kr = [[0.91 * w, 0, 0.5 * w + 1], [0, 0.9 * w, 0.5 * h - 1], [0, 0, 1]]
    return (rc.CameraModel(Kl, [-0.12, 0.03, 0.0005, -0.0003, 0.0]), rc.CameraModel(Kr, [-0.11, 0.02, -0.0004, 0.0002]),
            rc.rodrigues([0.004, -0.006, 0.003]), np.array([-0.25, 0.001, -0.002]))


def test_rectified_pair_feeds_the_chain_like_the_judges_arrays():
    m = _model()
    g = golden("c1_sceneflow")
    left, right = np.ascontiguousarray(g["left_u8"][:120, :300]), np.ascontiguousarray(g["right_u8"][:120, :300])
    cl, cr, R, T = _raw_rig((120, 300))
    rect = rc.stereo_rectify(cl, cr, R, T, (120, 300), out_size=(H, 300))
    pair = rc.Rectifier(rect, DEV, fill=0)(left, right, want_maps=True)
    jl, jr, jv = rj.rectify_judge(left[None], right[None], pair.maps.cpu().numpy()[None], 0)
    assert np.array_equal(pair.left.cpu().numpy(), jl[0]) and np.array_equal(pair.right.cpu().numpy(), jr[0])
    assert 0.5 < jv.mean() < 1.0
    a = kernels.standardize_crop_u8(pair.left, pair.right, H, W)
    b = kernels.standardize_crop_u8(_dev(jl[0]), _dev(jr[0]), H, W)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    kw = dict(tile=(H, W), context=8, ramp=8)
    sa = m.forward_scene(pair.left, pair.right, **kw)
    sb = m.forward_scene(jl[0], jr[0], **kw)
    assert sa.disp.shape == (H, 300) and torch.equal(sa.disp.view(torch.int32), sb.disp.view(torch.int32))
    cloud = kernels.reproject(sa.disp, rect.q(), pair.left, (pair.valid[0] == 0).to(torch.uint8))
    assert 0 < int(cloud.count) <= int(jv[0, 0].sum())


def test_predict_cli_calib(tmp_path):
    """A raw 120 x 300 pair through --calib: the rectified images are written on request, and
    the PLY is ``reproject`` of the written map with ``rect.q(origin)``, without the pixels
    --lr_check flags and the left pixels that have no source."""
    from PIL import Image
    from leastereo_amd import pointcloud as pc
    from leastereo_amd import predict as P
    g = golden("c1_sceneflow")
    for side in ("left", "right"):
        d = tmp_path / "frames_finalpass" / "S" / side
        d.mkdir(parents=True)
        Image.fromarray(g[side + "_u8"][:120, :300]).save(d / "0001.png")
    (tmp_path / "list.txt").write_text("S/left/0001.png\n")
    torch.save({"state_dict": {"module." + k: v for k, v in state_dict().items()}}, tmp_path / "ckpt.pth")
    cl, cr, R, T = _raw_rig((120, 300))
    rc.save_calibration(str(tmp_path / "rig.json"), cl, cr, R, T, (120, 300))
    base = ["--sceneflow=1", f"--maxdisp={MD}", "--crop_height=96", "--crop_width=192", f"--data_path={tmp_path}/",
            f"--test_list={tmp_path}/list.txt", f"--resume={tmp_path}/ckpt.pth", "--lr_check=1"]
    try:
        assert P.main(base + [f"--save_path={tmp_path}/out/", f"--calib={tmp_path}/rig.json", "--rect_fill=40",
                              "--save_rectified=1", "--pointcloud=1"]) == 0
    finally:
        P.set_rectifier(None)
    assert P.main(base + [f"--save_path={tmp_path}/plain/"]) == 0
    names = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert names == sorted([p.name for p in (tmp_path / "plain").iterdir()] +
                           ["0.ply", "0_rect_left.png", "0_rect_right.png", "0_rect_valid.png"])
    rect = rc.stereo_rectify(cl, cr, R, T, (120, 300))
    left, right = g["left_u8"][:120, :300], g["right_u8"][:120, :300]
    pair = kernels.rectify_u8(_dev(left), _dev(right), calib=rect.calib(), fill=40)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "0_rect_left.png")), pair.left.cpu().numpy())
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "0_rect_right.png")), pair.right.cpu().numpy())
    valid = np.asarray(Image.open(tmp_path / "out" / "0_rect_valid.png"))
    assert np.array_equal(valid, pair.valid[0].cpu().numpy() * 255) and 0 < (valid == 0).sum() < valid.size
    disp = np.load(tmp_path / "out" / "0.npy")
    assert not np.array_equal(disp, np.load(tmp_path / "plain" / "0.npy"))
    flagged = np.asarray(Image.open(tmp_path / "out" / "0_occ.png")) != 0
    x0, y0 = P.map_origin(120, 300, H, W)
    assert (x0, y0) == (54, 12) and disp.shape == (H, W)
    ex = flagged | (valid[y0:y0 + H, x0:x0 + W] == 0)
    want = kernels.reproject(_dev(disp), rect.q(origin=(x0, y0)), pair.left[y0:y0 + H, x0:x0 + W].contiguous(),
                             _dev(ex.astype(np.uint8))).to_host()
    xyz, rgb, nrm = pc.read_ply(tmp_path / "out" / "0.ply")
    assert nrm is None and 0 < len(xyz) == want.count < H * W
    assert np.array_equal(xyz.view(np.int32), want.xyz.view(np.int32)) and np.array_equal(rgb, want.rgb)
