"""The host side of rectification (leastereo_amd/rectify.py), the judges of tests/rectify_judge.py
against each other, and the new predict.py flags.  No GPU."""
import numpy as np
import pytest

from leastereo_amd import rectify as rc
from tests import rectify_judge as rj

SIZE = (480, 640)


def _cams(fl=520.0, fr=520.0):
    Kl = [[fl, 0, 318.2], [0, 1.01 * fl, 243.9], [0, 0, 1]]
    Kr = [[fr, 0, 325.7], [0, 0.99 * fr, 236.1], [0, 0, 1]]
    return rc.CameraModel(Kl, [0.1, -0.02, 0.001, 0.0005, 0.003]), rc.CameraModel(Kr, [0.09, -0.01, 0.0, 0.0007])


# name -> (R, T, stereo_rectify keywords, focal lengths)
RIGS = {
    "small": (rc.rodrigues([0.004, -0.007, 0.002]), [-0.12, 0.001, -0.002], {}, (520.0, 520.0)),
    "larger": (rc.rodrigues([0.11, -0.17, 0.09]), [-0.3, 0.04, -0.05], {}, (520.0, 520.0)),
    "toe_in": (rc.rodrigues([0.0, np.deg2rad(12.0), 0.0]), [-0.25, 0.0, 0.03], {}, (520.0, 520.0)),
    "unequal_focal": (rc.rodrigues([0.01, 0.02, -0.015]), [-0.5, -0.01, 0.02], {}, (480.0, 610.0)),
    "per_view_cx": (rc.rodrigues([-0.02, 0.05, 0.01]), [-0.2, 0.01, 0.0], dict(zero_disparity=False), (520.0, 500.0)),
    "resized": (rc.rodrigues([0.03, -0.04, 0.02]), [-0.15, 0.0, 0.01], dict(out_size=(300, 500)), (520.0, 530.0)),
    "resized_focal": (rc.rodrigues([0.0, 0.0, 0.05]), [-1.0, 0.1, 0.1], dict(out_size=(600, 700), focal=450.0,
                                                                            zero_disparity=False), (520.0, 520.0)),
    "identity": (np.eye(3), [-0.1, 0.0, 0.0], {}, (520.0, 520.0)),
}


def _rect(name):
    R, T, kw, (fl, fr) = RIGS[name]
    cl, cr = _cams(fl, fr)
    return rc.stereo_rectify(cl, cr, R, T, SIZE, **kw), R, np.asarray(T, float)


@pytest.mark.parametrize("name", list(RIGS))
def test_stereo_rectify_geometry(name):
    r, R, T = _rect(name)
    for Rk in (r.R1, r.R2):
        assert np.abs(Rk @ Rk.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rk) - 1) <= 1e-12
    nT = np.linalg.norm(T)
    assert np.abs(r.R2 @ T - np.array([-r.baseline, 0, 0])).max() <= 1e-12 * nT
    assert abs(r.baseline - nT) <= 1e-12 * nT
    kw = RIGS[name][2]
    assert r.size == SIZE and r.out_size == tuple(kw.get("out_size", SIZE))
    if kw.get("zero_disparity", True):
        assert r.cx == r.cx_right
    if "focal" in kw:
        assert r.focal == kw["focal"]
    else:
        fl, fr = RIGS[name][3]
        assert r.focal == pytest.approx(min(1.01 * fl, 0.99 * fr) * r.out_size[0] / SIZE[0], rel=1e-15)
    # random points in front of both cameras, in the left camera's frame
    rng = np.random.default_rng(3)
    X = np.stack([rng.uniform(-2, 2, 500), rng.uniform(-1.5, 1.5, 500), rng.uniform(3, 40, 500)])
    Xr = R @ X + T[:, None]
    assert (Xr[2] > 0).all()
    P1, P2 = r.projections()
    Xl_rect = r.R1 @ X
    h1 = P1 @ np.vstack([Xl_rect, np.ones(500)])
    h2 = P2 @ np.vstack([Xl_rect, np.ones(500)])
    # the same through each camera's own rotation: the right camera's rectified frame is the left's, shifted
    Xr_rect = r.R2 @ Xr
    assert np.abs(Xr_rect - (Xl_rect + np.array([[-r.baseline], [0], [0]]))).max() <= 1e-12 * 40
    K1, K2 = r.new_camera_matrices()
    g2 = K2 @ Xr_rect
    assert np.abs(g2 / g2[2] - h2 / h2[2]).max() <= 1e-9
    xl, yl = h1[0] / h1[2], h1[1] / h1[2]
    xr, yr = g2[0] / g2[2], g2[1] / g2[2]
    assert np.abs(yl - yr).max() <= 1e-9
    Z = Xl_rect[2]
    assert np.abs(xl - xr - (r.cx - r.cx_right) - r.focal * r.baseline / Z).max() <= 1e-9
    # Q (x, y, d, 1) returns R1 X
    h = r.q() @ np.stack([xl, yl, xl - xr, np.ones(500)])
    P = h[:3] / h[3]
    assert np.abs(P - Xl_rect).max() <= 1e-9 * np.abs(Xl_rect).max()
    # with an origin: the map's pixel (0, 0) at (x0, y0) of the rectified image
    h = r.q(origin=(17, 5)) @ np.stack([xl - 17, yl - 5, xl - xr, np.ones(500)])
    assert np.abs(h[:3] / h[3] - Xl_rect).max() <= 1e-9 * np.abs(Xl_rect).max()


@pytest.mark.parametrize("name", list(RIGS))
def test_calib_packs_the_inverse_of_the_new_projection(name):
    r, _, _ = _rect(name)
    c64 = r.calib64()
    c = r.calib()
    assert c.dtype == np.float32 and c.shape == (1, 2, 24) and np.array_equal(c[0], c64.astype(np.float32))
    for k, (Rk, Kn, cam) in enumerate(zip((r.R1, r.R2), r.new_camera_matrices(), (r.cam_l, r.cam_r))):
        M = c64[k, :9].reshape(3, 3)
        assert np.abs(Kn @ Rk @ M - np.eye(3)).max() <= 1e-12
        assert tuple(c64[k, 9:13]) == (cam.fx, cam.fy, cam.cx, cam.cy)
        assert c64[k, 13] == 0.0 and np.array_equal(c64[k, 14:22], cam.coefficients()) and not c64[k, 22:].any()
    assert np.array_equal(r.cam_l.coefficients(), [0.1, -0.02, 0.001, 0.0005, 0.003, 0, 0, 0])
    assert np.array_equal(r.cam_r.coefficients(), [0.09, -0.01, 0.0, 0.0007, 0, 0, 0, 0])
    f = rc.CameraModel(np.diag([300.0, 300.0, 1.0]), [0.1, 0.2, 0.3, 0.4], "fisheye")
    assert rc.stereo_rectify(f, f, np.eye(3), [-1, 0, 0], SIZE).calib64()[0, 13] == 1.0


def test_rodrigues_round_trip():
    rng = np.random.default_rng(0)
    for _ in range(50):
        om = rng.normal(size=3)
        om *= rng.uniform(0, 3.0) / np.linalg.norm(om)
        assert np.abs(rc.rodrigues_inv(rc.rodrigues(om)) - om).max() <= 1e-12
    assert np.array_equal(rc.rodrigues([0, 0, 0]), np.eye(3))
    assert np.abs(rc.rodrigues([0, 0, np.pi / 2]) - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() <= 1e-15


def test_vertical_and_swapped_rigs_are_refused():
    cl, cr = _cams()
    with pytest.raises(ValueError, match="vertical"):
        rc.stereo_rectify(cl, cr, np.eye(3), [-0.01, -0.2, 0.0], SIZE)
    with pytest.raises(ValueError, match="swapped"):
        rc.stereo_rectify(cl, cr, np.eye(3), [0.12, 0.0, 0.0], SIZE)
    with pytest.raises(ValueError):
        rc.stereo_rectify(cl, cr, np.eye(3), [0.0, 0.0, 0.0], SIZE)
    with pytest.raises(ValueError, match="focal"):
        rc.stereo_rectify(cl, cr, np.eye(3), [-0.1, 0, 0], SIZE, focal=-3.0)
    with pytest.raises(ValueError):
        rc.stereo_rectify(cl, cr, 2 * np.eye(3), [-0.1, 0, 0], SIZE)


def test_camera_model_refusals():
    K = [[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]
    for n in (4, 5, 8):
        assert rc.CameraModel(K, np.zeros(n)).dist.size == n
    assert rc.CameraModel(K, np.zeros(4), "fisheye").model == "fisheye"
    for n in (0, 3, 6, 7, 9, 12, 14):
        with pytest.raises(ValueError, match="distortion"):
            rc.CameraModel(K, np.zeros(n))
    for n in (5, 8):
        with pytest.raises(ValueError, match="distortion"):
            rc.CameraModel(K, np.zeros(n), "fisheye")
    with pytest.raises(ValueError, match="skew"):
        rc.CameraModel([[500.0, 0.3, 320], [0, 500, 240], [0, 0, 1]])
    with pytest.raises(ValueError):
        rc.CameraModel(K, model="thin_prism")
    with pytest.raises(ValueError):
        rc.CameraModel(np.eye(4))
    with pytest.raises(ValueError):
        rc.CameraModel([[-500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
    with pytest.raises(ValueError):
        rc.CameraModel(K, [np.nan, 0, 0, 0])


@pytest.mark.parametrize("ext", ["json", "npz"])
@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_calibration_files_round_trip(tmp_path, ext, model):
    cl, cr, R, T = rj.recipe_rig("fisheye" if model == "fisheye" else "rational8", SIZE)
    path = str(tmp_path / f"rig.{ext}")
    rc.save_calibration(path, cl, cr, R, T, SIZE)
    l2, r2, R2, T2, size = rc.load_calibration(path)
    assert size == SIZE and l2.model == r2.model == model
    for a, b in ((cl.K, l2.K), (cl.dist, l2.dist), (cr.K, r2.K), (cr.dist, r2.dist), (R, R2), (T, T2)):
        assert np.array_equal(a, b)            # repr of a float64 round-trips
    with pytest.raises(ValueError):
        rc.load_calibration(str(tmp_path / "rig.yaml"))
    with pytest.raises(ValueError):
        rc.save_calibration(str(tmp_path / "rig.yaml"), cl, cr, R, T, SIZE)


def test_calibration_file_with_a_missing_key(tmp_path):
    path = tmp_path / "bad.json"
    path.write_text('{"K1": [[1, 0, 0], [0, 1, 0], [0, 0, 1]]}')
    with pytest.raises(ValueError, match="lacks"):
        rc.load_calibration(str(path))


def test_predict_flags():
    from leastereo_amd import predict
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt"]
    off = obtain_predict_args(base)
    assert off.calib == "" and off.rect_size is None and off.rect_fill == 0 and off.save_rectified == 0
    assert predict.rectify_options(off) is None
    assert predict.rectify_options(obtain_predict_args(base + ["--rect_fill=999"])) is None   # off: not looked at
    # without --calib the point-cloud options are what they were
    pc_on = base + ["--pointcloud=1", "--pc_focal=400", "--pc_baseline=0.25"]
    assert predict.pointcloud_options(obtain_predict_args(pc_on)) == dict(
        focal=400.0, baseline=0.25, cx=None, cy=None, max_depth=0.0, normals=False)
    assert predict.load_pair.__doc__ and predict.last_rectified() is None
    on = base + ["--calib=rig.json"]
    assert predict.rectify_options(obtain_predict_args(on)) == dict(path="rig.json", size=None, fill=0, save=False)
    full = on + ["--rect_size", "300", "500", "--rect_fill=128", "--save_rectified=1"]
    assert predict.rectify_options(obtain_predict_args(full)) == dict(path="rig.json", size=(300, 500), fill=128,
                                                                      save=True)
    for bad in (["--rect_fill=256"], ["--rect_fill=-1"], ["--rect_size", "0", "5"]):
        with pytest.raises(ValueError):
            predict.rectify_options(obtain_predict_args(on + bad))
    with pytest.raises(NotImplementedError, match="--calib"):
        predict.rectify_options(obtain_predict_args(on + ["--satellite=1"]))
    # the rectification is the point cloud's calibration
    assert predict.pointcloud_options(obtain_predict_args(on + ["--pointcloud=1", "--pc_max_depth=20"])) == dict(
        focal=None, baseline=None, cx=None, cy=None, max_depth=20.0, normals=False)
    for flag in ("--pc_focal=400", "--pc_baseline=0.2", "--pc_cx=10", "--pc_cy=0"):
        with pytest.raises(ValueError, match=flag.split("=")[0]):
            predict.pointcloud_options(obtain_predict_args(on + ["--pointcloud=1", flag]))
    # main refuses before it needs a device
    with pytest.raises(ValueError, match="--pc_focal"):
        predict.main(on + ["--sceneflow=1", "--pointcloud=1", "--pc_focal=400"])
    with pytest.raises(ValueError, match="--rect_fill"):
        predict.main(on + ["--sceneflow=1", "--rect_fill=300"])


def test_load_pair_without_a_rectifier_is_load_images(tmp_path):
    from PIL import Image

    from leastereo_amd import predict
    img = rj.recipe_image((2, 9, 11), 3, seed=1)
    for k, name in enumerate(("l.png", "r.png")):
        Image.fromarray(img[k]).save(tmp_path / name)
    predict.set_rectifier(None)
    got = predict.load_pair(str(tmp_path / "l.png"), str(tmp_path / "r.png"))
    assert isinstance(got[0], np.ndarray) and np.array_equal(got[0], img[0]) and np.array_equal(got[1], img[1])


RECIPES = [((2, 61, 127), 3, (67, 131)), ((1, 40, 50), 4, (130, 70)), ((1, 2, 2), 3, (33, 40)), ((1, 1, 1), 4, (5, 3))]


@pytest.mark.parametrize("shape,ps,out", RECIPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pixel_judge_equals_float64_away_from_halves(shape, ps, out):
    """The float32 pixel judge is the float64 value rounded, wherever that value is not within
    1e-3 of a half; the recipe keeps the pixels left out at 1 % or fewer."""
    B, H, W = shape
    img = rj.recipe_image(shape, ps, seed=5)
    maps = rj.plant_specials(rj.smooth_warp(B, out[0], out[1], H, W, seed=9), H, W, seed=2, share=0.1)
    left_out = total = 0
    for b in range(B):
        for k in range(2):
            sx, sy = maps[b, k]
            got, valid = rj.pixel32(img[b], sx, sy, fill=171)
            v64, valid64 = rj.pixel64(img[b], sx, sy)
            assert np.array_equal(valid != 0, valid64)
            assert (got[valid == 0] == 171).all()
            near = np.abs(v64 - np.floor(v64) - 0.5) <= 1e-3
            clear = valid64[..., None] & ~near
            assert np.array_equal(got[clear], np.rint(v64[clear]).astype(np.uint8))
            assert np.abs(got[valid64].astype(np.float64) - v64[valid64]).max(initial=0) <= 0.5 + 1e-3
            left_out += int((near.any(-1) & valid64).sum())
            total += int(valid64.sum())
    assert total > 0 and left_out <= 0.01 * total, (left_out, total)


def test_pixel_judge_on_a_hand_case():
    img = np.array([[[10], [20], [40]], [[50], [70], [110]]], np.uint8).repeat(3, -1)
    f = np.float32
    sx = np.array([[0, 2, 0.5, 1.25, 2.0000002, -0.0, -1e-6, np.nan, 1, 0.5]], f)
    sy = np.array([[0, 1, 0, 0.5, 0, 1, 0, 0, np.inf, 0.75]], f)
    out, valid = rj.pixel32(img, sx, sy, fill=7)
    assert valid.tolist() == [[1, 1, 1, 1, 0, 1, 0, 0, 0, 1]]
    #  (0,0)=10; (2,1)=110; 15; top=25 bot=80 -> 52.5 -> 52 (half to even); fill; (0,1)=50; fill x3; top=15 bot=60 -> 48.75
    assert out[0, :, 0].tolist() == [10, 110, 15, 52, 7, 50, 7, 7, 7, 49]
    assert (out == out[..., :1]).all()


def test_map_judges_agree_and_mark_the_same_pixels():
    """The float32 restatement against the float64 judge on the recipe rigs: the same NaN pattern
    and an error of the order the issue quotes (1e-4 px at 576 x 960; less at these sizes)."""
    for name in rj.RIGS:
        cl, cr, R, T = rj.recipe_rig(name, (61, 127))
        r = rc.stereo_rectify(cl, cr, R, T, (61, 127), out_size=(67, 131))
        c = r.calib()[0]
        m64, m32 = rj.map64(c, 67, 131), rj.map32(c, 67, 131)
        assert m32.dtype == np.float32 and np.array_equal(np.isnan(m64), np.isnan(m32))
        assert np.isfinite(m64).all()
        assert np.abs(m32 - m64).max() <= 1e-3
        # the maps cover the raw image: most rectified pixels have a source
        inside = (m64[:, 0] >= 0) & (m64[:, 0] <= 126) & (m64[:, 1] >= 0) & (m64[:, 1] <= 60)
        assert inside.mean() > 0.6, (name, inside.mean())
    c = rj.behind_calib(67, 131)
    m64, wc = rj.map64(c, 67, 131, return_wc=True)
    assert np.abs(wc).min() > 1e-3 and 0.05 < np.isnan(m64[:, 0]).mean() < 0.95
    assert np.array_equal(np.isnan(m64), np.isnan(rj.map32(c, 67, 131)))


def test_zero_distortion_identity_maps_are_the_pixel_grid():
    cam = rc.CameraModel([[256.0, 0, 40], [0, 256.0, 30], [0, 0, 1]])
    r = rc.stereo_rectify(cam, cam, np.eye(3), [-0.1, 0, 0], (61, 81))
    assert (r.focal, r.cx, r.cy, r.cx_right) == (256.0, 40.0, 30.0, 40.0)
    m = rj.map32(r.calib()[0], 61, 81)
    v, u = np.meshgrid(np.arange(61, dtype=np.float32), np.arange(81, dtype=np.float32), indexing="ij")
    assert np.array_equal(m[0, 0], u) and np.array_equal(m[1, 1], v)
