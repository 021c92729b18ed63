"""The host side of the point cloud, without a device: the judge of tests/pointcloud_judge.py
against the closed form of a rectified rig, ``pointcloud.q_matrix`` / ``write_ply`` /
``read_ply``, the predict.py flags, and the judge's own order and truncation on a hand case."""
import numpy as np
import pytest

from leastereo_amd import pointcloud as pc
from tests import pointcloud_judge as pj

SHAPES = [(2, 67, 131), (1, 130, 70), (1, 33, 129)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_judge_is_the_closed_form_on_the_recipe(shape):
    """Z = f B / d, X = (x - cx) Z / f, Y = (y - cy) Z / f in float64 where the pixel is valid; the
    recipe's statistics (valid share, normals, conditioning) are what the GPU tests rely on."""
    B, H, W = shape
    d, e = pj.slanted_field(shape, seed=sum(shape))
    out = pj.judge(d, pj.recipe_q(H, W), None, e, normals=True)
    ok = (e == 0) & np.isfinite(d) & (d > 0)
    assert np.array_equal(out["valid"], ok.astype(np.uint8)) and np.array_equal(out["count"], ok.reshape(B, -1).sum(1))
    assert 0.93 < ok.mean() < 0.97
    y, x = np.mgrid[:H, :W]
    with np.errstate(all="ignore"):
        Z = pj.F * pj.BASELINE / d.astype(np.float64)
        want = np.stack([(x - W / 2) * Z / pj.F, (y - H / 2) * Z / pj.F, Z], -1)
    got = out["points"]
    assert np.isnan(got[~ok]).all() and np.isfinite(got[ok]).all()
    assert np.abs(got[ok] - want[ok]).max() <= 1e-12 * np.abs(want[ok]).max()
    # the float32 restatement: the same validity, the same pixels with a normal
    f32 = pj.judge(d, pj.recipe_q(H, W), None, e, normals=True, dtype=np.float32)
    assert np.array_equal(f32["valid"], out["valid"]) and f32["points"].dtype == np.float32
    dg = out["diag"]
    assert np.array_equal(dg["has"], f32["diag"]["has"])
    assert dg["has"][ok].mean() > 0.95 and not dg["has"][~ok].any()
    assert np.nanmin(dg["cos"]) > 1e-2 and np.nanmin(dg["rel"]) > 1e-2
    rel = np.abs(f32["points"][ok].astype(np.float64) - got[ok]).max() / np.abs(got[ok]).max()
    nerr = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(f32["normals"], out["normals"]))
    print(f"{shape}: {100 * ok.mean():.1f} % valid, {100 * dg['has'][ok].mean():.1f} % of them with a normal, min |cos| "
          f"{np.nanmin(dg['cos']):.3f}, float32 restatement: points {rel:.1e} relative, normals {nerr:.1e}")
    assert rel < 5e-7 and nerr < 1e-3
    for n in out["normals"]:                      # unit length or none, towards the camera
        ln = np.sqrt((n ** 2).sum(1))
        assert (np.abs(ln[ln > 0] - 1) < 1e-12).all()
    for b in range(B):
        has = out["normals"][b].any(1)
        assert ((out["normals"][b] * out["xyz"][b]).sum(1)[has] < 0).all()


def test_q_matrix_with_an_origin_is_a_pixel_translation():
    Q = pc.q_matrix(721.5, 0.54, 609.6, 172.9)
    assert Q.dtype == np.float64 and Q.shape == (4, 4)
    T = np.eye(4)
    T[0, 3], T[1, 3] = 37.0, 12.0
    assert np.array_equal(pc.q_matrix(721.5, 0.54, 609.6, 172.9, origin=(37, 12)), Q @ T)
    # the definition, with a right principal point
    Q = pc.q_matrix(400.0, 0.25, 64.0, 32.0, cx_right=61.0, origin=(5, 7))
    x, y, d = 10.0, 20.0, 13.0
    h = Q @ np.array([x, y, d, 1.0])
    Z = 400.0 * 0.25 / (d - 3.0)
    assert np.allclose(h[:3] / h[3], [(x + 5 - 64.0) * Z / 400.0, (y + 7 - 32.0) * Z / 400.0, Z], rtol=1e-15)
    for bad in (dict(focal=0.0), dict(focal=float("nan")), dict(baseline=-1.0), dict(baseline=float("inf"))):
        with pytest.raises(ValueError):
            pc.q_matrix(**dict(dict(focal=400.0, baseline=0.25, cx=1.0, cy=1.0), **bad))


@pytest.mark.parametrize("with_rgb", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
def test_ply_round_trip_is_bit_for_bit(tmp_path, with_rgb, with_normals):
    rng = np.random.default_rng(5)
    n = 77
    xyz = rng.integers(0, 2 ** 32, (n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)   # any bits, NaNs too
    nrm = rng.integers(0, 2 ** 32, (n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32) if with_normals else None
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8) if with_rgb else None
    path = tmp_path / "c.ply"
    size = pc.write_ply(path, xyz, rgb, nrm)
    data = path.read_bytes()
    want = "ply\nformat binary_little_endian 1.0\nelement vertex 77\nproperty float x\nproperty float y\nproperty float z\n"
    if with_normals:
        want += "property float nx\nproperty float ny\nproperty float nz\n"
    if with_rgb:
        want += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    want += "end_header\n"
    assert data.startswith(want.encode()) and pc.ply_header(n, with_rgb, with_normals) == want
    assert size == len(data) == len(want) + n * (12 + (12 if with_normals else 0) + (3 if with_rgb else 0))
    # the first vertex, by hand
    first = data[len(want):len(want) + 12]
    assert first == xyz[0].astype("<f4").tobytes()
    x2, c2, n2 = pc.read_ply(path)
    assert x2.dtype == np.float32 and np.array_equal(x2.view(np.uint32), xyz.view(np.uint32))
    assert (c2 is None) == (rgb is None) and (n2 is None) == (nrm is None)
    if with_rgb:
        assert c2.dtype == np.uint8 and np.array_equal(c2, rgb)
    if with_normals:
        assert np.array_equal(n2.view(np.uint32), nrm.view(np.uint32))


def test_ply_empty_cloud_and_refusals(tmp_path):
    path = tmp_path / "e.ply"
    pc.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    x, c, n = pc.read_ply(path)
    assert x.shape == (0, 3) and c.shape == (0, 3) and n is None
    for bad in (dict(xyz=np.zeros((4, 3))), dict(xyz=np.zeros((4, 2), np.float32)),
                dict(xyz=np.zeros((4, 3), np.float32), rgb=np.zeros((3, 3), np.uint8)),
                dict(xyz=np.zeros((4, 3), np.float32), rgb=np.zeros((4, 3), np.float32)),
                dict(xyz=np.zeros((4, 3), np.float32), normals=np.zeros((4, 3)))):
        with pytest.raises(ValueError):
            pc.write_ply(tmp_path / "bad.ply", **bad)
    (tmp_path / "short.ply").write_bytes(path.read_bytes().replace(b"vertex 0", b"vertex 2"))
    with pytest.raises(ValueError):
        pc.read_ply(tmp_path / "short.ply")
    (tmp_path / "ascii.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        pc.read_ply(tmp_path / "ascii.ply")


def test_predict_flags():
    from leastereo_amd import predict
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt"]
    assert predict.pointcloud_options(obtain_predict_args(base)) is None
    assert predict.pointcloud_options(obtain_predict_args(base + ["--pc_focal=-1"])) is None   # off: nothing is looked at
    on = base + ["--pointcloud=1", "--pc_focal=400", "--pc_baseline=0.25"]
    assert predict.pointcloud_options(obtain_predict_args(on)) == dict(
        focal=400.0, baseline=0.25, cx=None, cy=None, max_depth=0.0, normals=False)
    full = on + ["--pc_cx=100.5", "--pc_cy=50", "--pc_max_depth=20", "--pc_normals=1"]
    assert predict.pointcloud_options(obtain_predict_args(full)) == dict(
        focal=400.0, baseline=0.25, cx=100.5, cy=50.0, max_depth=20.0, normals=True)
    for bad in (["--pointcloud=1"], ["--pointcloud=1", "--pc_focal=400"], ["--pointcloud=1", "--pc_baseline=0.25"],
                ["--pointcloud=1", "--pc_focal=0", "--pc_baseline=0.25"],
                ["--pointcloud=1", "--pc_focal=400", "--pc_baseline=-0.25"],
                ["--pointcloud=1", "--pc_focal=nan", "--pc_baseline=0.25"],
                ["--pointcloud=1", "--pc_focal=400", "--pc_baseline=inf"],
                on[4:] + ["--pc_max_depth=-1"], on[4:] + ["--pc_max_depth=nan"], on[4:] + ["--pc_cx=inf"]):
        with pytest.raises(ValueError):
            predict.pointcloud_options(obtain_predict_args(base + bad))
    with pytest.raises(NotImplementedError):
        predict.pointcloud_options(obtain_predict_args(on + ["--satellite=1"]))
    # main refuses before it needs a device
    with pytest.raises(ValueError, match="--pc_focal"):
        predict.main(base + ["--sceneflow=1", "--pointcloud=1", "--pc_baseline=0.25"])
    with pytest.raises(NotImplementedError, match="--pointcloud"):
        predict.main(on + ["--satellite=1"])


def test_map_origin_is_where_the_written_map_lies():
    from leastereo_amd import predict
    assert predict.map_origin(540, 960, 540, 960) == (0, 0)            # fits the crop, or --scene
    assert predict.map_origin(540, 960, 384, 576) == (192, 78)         # the centre crop
    assert predict.map_origin(541, 961, 384, 576) == (192, 78)         # int((h - ch) / 2), as main cuts the GT
    for h, w, ch, cw in ((540, 960, 384, 576), (541, 961, 96, 192)):    # crop_output's own slice of a larger image
        img = np.arange(h * w).reshape(h, w)
        sy, sx = (h - ch) // 2, (w - cw) // 2                           # test_transform's centre crop
        x0, y0 = predict.map_origin(h, w, ch, cw)
        assert np.array_equal(img[sy:sy + ch, sx:sx + cw], img[y0:y0 + ch, x0:x0 + cw])


def test_judge_order_and_truncation_on_a_hand_case():
    d = np.array([[1, 0, 2, np.nan, 4],
                  [5, 5, -1, 8, 8],
                  [np.inf, 2, 2, 2, 16]], np.float32)
    e = np.zeros((3, 5), np.uint8)
    e[1, 1], e[2, 3] = 1, 200
    Q = pc.q_matrix(2.0, 1.0, 0.0, 0.0)                 # Z = 2 / d, X = x Z / 2, Y = y Z / 2
    image = np.arange(3 * 5 * 4, dtype=np.uint8).reshape(3, 5, 4)
    out = pj.judge(d, Q, image, e, max_disp=8.0)
    want = [0, 2, 4, 5, 8, 9, 11, 12]                   # row-major; 16 > max_disp, 0 and -1 <= min_disp
    assert out["count"].tolist() == [8] and out["index"][0].tolist() == want
    assert np.array_equal(out["valid"][0].ravel().nonzero()[0], want)
    assert np.array_equal(out["xyz"][0][1], [2 * (2 / 2.0) / 2, 0.0, 2 / 2.0])          # pixel (2, 0), d = 2
    assert np.array_equal(out["xyz"][0][6], [1 * (2 / 2.0) / 2, 2 * (2 / 2.0) / 2, 1.0])  # pixel (1, 2), d = 2
    assert np.array_equal(out["rgb"][0], image.reshape(15, 4)[want, :3])
    for cap in (1, 7, 8, 9, 15):
        cut = pj.judge(d, Q, image, e, max_disp=8.0, capacity=cap)
        assert cut["count"].tolist() == [8]             # the count is not cut
        assert cut["index"][0].tolist() == want[:cap] and len(cut["xyz"][0]) == min(cap, 8)
        assert np.array_equal(cut["xyz"][0], out["xyz"][0][:cap]) and np.array_equal(cut["rgb"][0], out["rgb"][0][:cap])
    # absent differences: pixel 12 = (2, 2) has a usable left neighbour along x ((3, 2) is excluded), but
    # none along y ((2, 1) holds -1 and is not valid, (2, 3) is outside)
    n = pj.judge(d, Q, None, e, max_disp=8.0, normals=True, normal_max_diff=0.5)
    assert n["normals"][0][want.index(12)].tolist() == [0.0, 0.0, 0.0]
    assert n["normals"][0][want.index(0)].tolist() == [0.0, 0.0, 0.0]      # pixel (0, 0): no usable neighbour
