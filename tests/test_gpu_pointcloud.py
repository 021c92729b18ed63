"""The point cloud on the GPU (lea_disparity_pointcloud_f32, kernels.reproject,
LEAStereo.forward_points / graphed(points=...), scene.points_scene, predict.py --pointcloud).

BLK = 1024: the pixels of a workgroup of the count and scatter launches (256 lanes x 4 pixels; a
wave takes 64 consecutive pixels at a time).  SCAN = 1024: the block counts one pass of the scan
workgroup takes (256 lanes x 4 counts).  The shapes: a pixel, a row, a column, the three fields
of the other heads' tests, exactly 2 BLK pixels, three images of two blocks each, and one row
of SCAN * BLK + BLK + 3 pixels, where the scan takes a second pass that ends on a partial block.

Every case compares with tests/pointcloud_judge.py, no pixel left out:
  * valid, count, index, rgb and the NaN pattern of points bit for bit; every compact row at or
    beyond min(count, capacity) still holds the sentinel it was filled with (0x7fc0dead in the
    four-byte arrays, 0xAB in rgb), and so do 256 elements either side of every output;
  * xyz equals the points rows at index bit for bit (one copy of the arithmetic in the kernel);
  * the largest error of points / xyz against the float64 judge is at most
    max(4 x the float32 restatement's largest error in that case, 8 ulp of the case's largest
    coordinate), the standing bar of the float heads; the normals are held to the same bar, and
    which rows are (0, 0, 0) equals the judge exactly.  Before a case's normals are compared, the
    judge itself must show no |cos(n, P)| below 1e-3 and no cross product below 1e-6 |dx| |dy|:
    no orientation flip and no zero test of the case is then a matter of rounding.
"""
import functools

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels, scene
from leastereo_amd import pointcloud as pc
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from tests import pointcloud_judge as pj
from tests.golden_util import golden, normal, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLK, SCAN = 1024, 1024
BIG = (1, 1, SCAN * BLK + BLK + 3)
SHAPES = [(1, 1, 1), (1, 1, 257), (1, 33, 1), (2, 67, 131), (1, 130, 70), (1, 33, 129), (1, 32, 64), (3, 40, 50), BIG]
PATTERNS = ["all", "none", "last", "checkerboard", "runs64", "runs64_offset", "recipe", "random1"]
IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
SENT, SENT_BYTE, GUARD = 0x7FC0DEAD, 0xAB, 256


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)  # a copy: the references are read-only


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def field(shape):
    """The recipe's field, its exclude bytes, a clean copy of the field (every pixel finite and
    above 0) and an image, shared and read-only."""
    d, e = pj.slanted_field(shape, seed=sum(shape))
    if shape == BIG:  # a block of W / 6 pixels would run its plane far below 0: rows of 256 of the recipe, end to end
        d = pj.slanted_field((-(-shape[2] // 256), 1, 256), seed=3)[0].reshape(1, 1, -1)[:, :, :shape[2]]
    clean = np.where(np.isfinite(d) & (d > 0), d, np.float32(20.0)).astype(np.float32)
    img = pj.recipe_image(shape, seed=sum(shape))
    for a in (d, e, clean, img):
        a.setflags(write=False)
    return d, e, clean, img


def pattern(shape, name):
    """(disp, exclude) of a validity pattern on the clean field."""
    d, e, clean, _ = field(shape)
    B, H, W = shape
    i = np.arange(H * W).reshape(H, W)
    if name == "recipe":
        return d, e
    if name == "all":
        return clean, None
    if name == "none":
        ex = np.ones(shape, bool)
    elif name == "last":
        ex = np.ones(shape, bool)
        ex[:, -1, -1] = False
    elif name == "checkerboard":
        ex = np.broadcast_to((i // W + i % W) % 2 == 1, shape)
    elif name == "runs64":
        ex = np.broadcast_to((i // 64) % 2 == 1, shape)
    elif name == "runs64_offset":
        ex = np.broadcast_to(((i + 1) // 64) % 2 == 1, shape)
    else:
        ex = np.random.default_rng(7).random(shape) >= 0.01
    return clean, np.where(ex, 1 + (i % 3), 0).astype(np.uint8)


def run_raw(d, Q, image=None, exclude=None, min_disp=0.0, max_disp=np.inf, nmd=1.0, capacity=None, normals=True):
    """The C entry with every output asked for, in buffers filled with the sentinels and with
    guard bands; the arrays as numpy, the compact ones [B, capacity, ...]."""
    d = np.asarray(d, np.float32)
    B, H, W = d.shape
    cap = H * W if capacity is None else capacity
    lib = _lib.load()
    dd, ee, ii = _dev(d), _dev(exclude), _dev(image)
    q = torch.from_numpy(np.asarray(Q, np.float64).astype(np.float32).reshape(-1, 16)).to(DEV)
    wsn = lib.lea_disparity_pointcloud_workspace_bytes(B, H, W)
    assert wsn == 4 * B * -(-(H * W) // BLK)
    n = B * H * W
    sizes = dict(ws=(wsn // 4, torch.int32), points=(3 * n, torch.int32), valid=(n, torch.uint8),
                 count=(B, torch.int32), xyz=(3 * B * cap, torch.int32), rgb=(3 * B * cap, torch.uint8),
                 index=(B * cap, torch.int32), normals=(3 * B * cap, torch.int32))
    if image is None:
        del sizes["rgb"]
    if not normals:
        del sizes["normals"]
    bufs = {k: torch.full((m + 2 * GUARD,), SENT if t == torch.int32 else SENT_BYTE, device=DEV, dtype=t)
            for k, (m, t) in sizes.items()}
    p = {k: v.data_ptr() + GUARD * v.element_size() for k, v in bufs.items()}
    kernels.check(lib.lea_disparity_pointcloud_f32(
        dd.data_ptr(), None if ee is None else ee.data_ptr(), None if ii is None else ii.data_ptr(),
        0 if image is None else image.shape[-1], q.data_ptr(), 16 if q.shape[0] > 1 else 0, B, H, W, float(min_disp),
        float(max_disp), float(nmd), cap, p["ws"], p["points"], p["valid"], p["count"], p["xyz"], p.get("rgb"),
        p["index"], p.get("normals"), None), "pointcloud")
    torch.cuda.synchronize()
    out = {}
    for k, v in bufs.items():
        a = v.cpu().numpy()
        s = SENT if a.dtype == np.int32 else SENT_BYTE
        assert (a[:GUARD] == s).all() and (a[-GUARD:] == s).all(), f"{k}: a guard band was written"
        out[k] = a[GUARD:-GUARD]
    assert np.array_equal(_bits(dd), _bits(d))                       # the inputs too
    assert exclude is None or np.array_equal(ee.cpu().numpy(), exclude)
    out["points"] = out["points"].reshape(B, H, W, 3)
    out["valid"] = out["valid"].reshape(B, H, W)
    for k in ("xyz", "rgb", "normals"):
        if k in out:
            out[k] = out[k].reshape(B, cap, 3)
    out["index"] = out["index"].reshape(B, cap)
    return out


def bar(j32, j64):
    """max(4 x the float32 restatement's largest error, 8 ulp of the largest coordinate)."""
    if j64.size == 0:
        return 0.0
    err32 = float(np.abs(j32.astype(np.float64) - j64).max())
    return max(4.0 * err32, 8.0 * float(np.spacing(np.float32(np.abs(j64).max()))))


def assert_is_judge(raw, d, Q, image=None, exclude=None, min_disp=0.0, max_disp=np.inf, nmd=1.0, capacity=None,
                    normals=True, what=""):
    B, H, W = np.asarray(d).shape
    cap = H * W if capacity is None else capacity
    kw = dict(image=image, exclude=exclude, min_disp=min_disp, max_disp=max_disp, normals=normals,
              normal_max_diff=nmd, capacity=cap)
    j64, j32 = pj.judge(d, Q, **kw), pj.judge(d, Q, dtype=np.float32, **kw)
    assert np.array_equal(j32["valid"], j64["valid"]), what
    ok = j64["valid"].astype(bool)
    assert np.array_equal(raw["valid"], j64["valid"]), f"{what} valid: {(raw['valid'] != j64['valid']).sum()} differ"
    assert np.array_equal(raw["count"], j64["count"]), (what, raw["count"], j64["count"])
    pts = raw["points"].view(np.float32)
    assert np.array_equal(np.isnan(pts), np.isnan(j64["points"])), what
    assert (raw["points"][~ok] == 0x7FC00000).all(), f"{what}: an invalid pixel is not the quiet NaN"
    perr = float(np.abs(pts[ok].astype(np.float64) - j64["points"][ok]).max()) if ok.any() else 0.0
    pbar = bar(j32["points"][ok], j64["points"][ok])
    print(f"{what}: {int(ok.sum())} of {ok.size} valid; points: error {perr:.3g}, bar {pbar:.3g}", end="")
    assert perr <= pbar, (what, perr, pbar)
    if normals and j64["diag"]["both"].any():  # the judge's own conditioning, before any normal is compared
        dg = j64["diag"]
        assert not (dg["cos"][dg["has"]] < 1e-3).any(), f"{what}: the case has an ambiguous orientation"
        assert not (dg["rel"][dg["both"]] < 1e-6).any(), f"{what}: the case has a degenerate cross product"
        assert np.array_equal(dg["has"], j32["diag"]["has"]), what
    for b in range(B):
        rows = min(int(j64["count"][b]), cap)
        assert len(j64["index"][b]) == rows
        idx = j64["index"][b]
        assert np.array_equal(raw["index"][b, :rows], idx), f"{what} item {b}: index"
        assert (raw["index"][b, rows:] == SENT).all(), f"{what} item {b}: an index row beyond the count was written"
        assert np.array_equal(raw["xyz"][b, :rows], raw["points"][b].reshape(-1, 3)[idx]), f"{what} item {b}: xyz"
        assert (raw["xyz"][b, rows:] == SENT).all(), f"{what} item {b}: an xyz row beyond the count was written"
        if image is not None:
            assert np.array_equal(raw["rgb"][b, :rows], j64["rgb"][b]), f"{what} item {b}: rgb"
            assert (raw["rgb"][b, rows:] == SENT_BYTE).all(), f"{what} item {b}: an rgb row beyond the count was written"
        if normals:
            got = raw["normals"][b, :rows].view(np.float32)
            assert (raw["normals"][b, rows:] == SENT).all(), f"{what} item {b}: a normal beyond the count was written"
            assert np.array_equal((got == 0).all(1), (j64["normals"][b] == 0).all(1)), f"{what} item {b}: which normals"
            nerr = float(np.abs(got.astype(np.float64) - j64["normals"][b]).max()) if rows else 0.0
            nbar = bar(j32["normals"][b], j64["normals"][b])
            print(f"; item {b} normals: {int((got != 0).any(1).sum())} of {rows}, error {nerr:.3g}, bar {nbar:.3g}", end="")
            assert nerr <= nbar, (what, b, nerr, nbar)
    print()
    return j64


# ------------------------------------------------------------------ shapes x validity patterns
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_patterns(shape, name):
    d, e = pattern(shape, name)
    B, H, W = shape
    Q = pj.recipe_q(H, W)
    img = field(shape)[3]
    if B > 1:                                   # three bytes a pixel for the batches, four (one unread) elsewhere
        img = np.ascontiguousarray(img[..., :3])
    normals = H > 1 and W > 1 or H * W < BLK    # a long line has none, as the short lines show
    raw = run_raw(d, Q, img, e, normals=normals)
    j = assert_is_judge(raw, d, Q, img, e, normals=normals, what=f"{shape} {name}")
    n = j["count"]
    if name == "all":
        assert (n == H * W).all()
    if name == "none":
        assert (n == 0).all()
    if name == "last":
        assert (n == 1).all() and all(i.tolist() == [H * W - 1] for i in j["index"])
    if name == "recipe" and H * W >= 2000 and H > 1:
        ok = j["valid"].astype(bool)
        assert 0.93 < ok.mean() < 0.97 and j["diag"]["has"][ok].mean() > 0.95


def test_batch_matrices_and_2d_wrapper():
    """A matrix per image (stride 16), and the wrapper on a [H, W] map without a batch axis."""
    shape = (3, 40, 50)
    d, e = pattern(shape, "recipe")
    Q = np.stack([pj.recipe_q(40, 50), pc.q_matrix(300.0, 0.1, 20.0, 30.0, origin=(3, 4)),
                  pc.q_matrix(500.0, 1.5, 25.0, 20.0, cx_right=24.0)])
    raw = run_raw(d, Q, None, e)
    assert_is_judge(raw, d, Q, None, e, what="three matrices")
    cloud = kernels.reproject(_dev(d[1]), Q[1], exclude=_dev(e[1]), normals=True, want_points=True, want_valid=True)
    assert cloud.points.shape == (40, 50, 3) and cloud.count.shape == () and cloud.rgb is None
    host = cloud.to_host()
    one = run_raw(d[1:2], Q[1], None, e[1:2])
    assert host.count == one["count"][0] and host.rgb is None
    assert np.array_equal(_bits(host.xyz), one["xyz"][0, :host.count])
    assert np.array_equal(_bits(host.normals), one["normals"][0, :host.count])
    assert np.array_equal(host.index, one["index"][0, :host.count])
    assert np.array_equal(_bits(cloud.points), one["points"][0]) and np.array_equal(cloud.valid.cpu().numpy(), one["valid"][0])


# ------------------------------------------------------------------ capacity
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_capacity_around_the_count(delta):
    shape = (2, 67, 131)
    d, e = pattern(shape, "recipe")
    Q, img = pj.recipe_q(67, 131), field(shape)[3]
    counts = pj.judge(d, Q, exclude=e)["count"]
    assert counts[0] != counts[1]
    cap = int(counts.min()) + delta          # the other image overflows by more
    raw = run_raw(d, Q, img, e, capacity=cap)
    j = assert_is_judge(raw, d, Q, img, e, capacity=cap, what=f"capacity {cap} for counts {counts.tolist()}")
    assert np.array_equal(j["count"], counts)                       # the count is not cut


def test_capacity_with_no_row_needed_and_one_row():
    shape = (2, 67, 131)
    d, e = pattern(shape, "none")
    Q = pj.recipe_q(67, 131)
    for cap in (1, 5):
        assert_is_judge(run_raw(d, Q, None, e, capacity=cap), d, Q, None, e, capacity=cap, what=f"none valid, capacity {cap}")
    d, e = pattern(shape, "all")
    assert_is_judge(run_raw(d, Q, None, e, capacity=1), d, Q, None, e, capacity=1, what="all valid, capacity 1")
    assert_is_judge(run_raw(d, Q, None, e, capacity=BLK + 1), d, Q, None, e, capacity=BLK + 1, what="all valid, BLK + 1")


# ------------------------------------------------------------------ values
def test_disparity_range_and_non_finite_values():
    d = np.array(field((1, 33, 129))[2])
    d[0, 3, 5:9] = [np.inf, -np.inf, np.nan, -0.0]
    d[0, 7, 7], d[0, 8, 8] = 12.0, np.nextafter(np.float32(12.0), np.float32(13.0))
    d[0, 9, 9], d[0, 10, 10] = 40.0, np.nextafter(np.float32(40.0), np.float32(41.0))
    Q = pj.recipe_q(33, 129)
    raw = run_raw(d, Q, None, None, min_disp=12.0, max_disp=40.0)
    assert_is_judge(raw, d, Q, None, None, min_disp=12.0, max_disp=40.0, what="12 < d <= 40")
    v = raw["valid"][0]
    assert (v[3, 5:9] == 0).all() and v[7, 7] == 0 and v[8, 8] == 1 and v[9, 9] == 1 and v[10, 10] == 0
    raw = run_raw(d, Q, None, None, min_disp=-np.inf, max_disp=np.inf)
    assert_is_judge(raw, d, Q, None, None, min_disp=-np.inf, what="every finite disparity")
    assert raw["valid"][0][3, 8] == 0 and np.isnan(raw["points"].view(np.float32)[0, 3, 8]).all()   # d = -0: h3 = 0


def test_degenerate_matrix_h3_exactly_zero():
    """q32 = 1, q33 = -2: h3 = d - 2 is exactly 0 at d = 2 whatever the contraction; that pixel
    is invalid (its coordinates are not finite) and no other pixel moves."""
    d = np.array(field((1, 33, 129))[2])
    where = [(0, 0), (5, 63), (5, 64), (32, 128)]
    for y, x in where:
        d[0, y, x] = 2.0
    Q = np.array([[1, 0, 0, -64.5], [0, 1, 0, -16.5], [0, 0, 0, 400.0], [0, 0, 1, -2]], np.float64)
    raw = run_raw(d, Q)
    j = assert_is_judge(raw, d, Q, what="h3 = 0")
    assert j["count"][0] == 33 * 129 - len(where)
    for y, x in where:
        assert raw["valid"][0, y, x] == 0 and (raw["points"][0, y, x] == 0x7FC00000).all()
    d2 = np.array(d)
    for y, x in where:
        d2[0, y, x] = 3.0
    other = run_raw(d2, Q, normals=False)
    keep = np.ones((33, 129), bool)
    for y, x in where:
        keep[y, x] = False
    assert np.array_equal(raw["points"][0][keep], other["points"][0][keep])


def test_one_sided_differences_across_a_disparity_step():
    """Two fronto-parallel planes, d = 10 left of x = 4 and d = 20 from there on, a step above
    normal_max_diff = 1: the columns either side of the step take the one-sided difference
    inside their own plane, so every normal is (0, 0, -1); with normal_max_diff = 10 the step's
    two columns difference across it and tilt."""
    d = np.full((1, 6, 8), 10.0, np.float32)
    d[:, :, 4:] = 20.0
    Q = pc.q_matrix(100.0, 1.0, 4.0, 3.0)
    raw = run_raw(d, Q, nmd=1.0)
    assert_is_judge(raw, d, Q, nmd=1.0, what="step, max diff 1")
    n = raw["normals"][0].view(np.float32).reshape(6, 8, 3)
    assert np.array_equal(n[..., 2], np.full((6, 8), -1.0, np.float32)) and (n[..., :2] == 0).all()
    raw = run_raw(d, Q, nmd=10.0)
    assert_is_judge(raw, d, Q, nmd=10.0, what="step, max diff 10")
    n = raw["normals"][0].view(np.float32).reshape(6, 8, 3)
    assert (n[:, [0, 1, 2, 5, 6, 7], 2] == -1.0).all() and (np.abs(n[:, 3:5, 0]) > 0.5).all()
    # a single row or column has no second direction: no normal anywhere
    for shape in ((1, 1, 9), (1, 9, 1)):
        line = np.full(shape, 10.0, np.float32)
        raw = run_raw(line, Q)
        assert_is_judge(raw, line, Q, what=f"{shape}")
        assert (raw["normals"].view(np.float32) == 0).all()


# ------------------------------------------------------------------ plumbing
def test_two_calls_give_identical_bits():
    shape = (2, 67, 131)
    d, e = pattern(shape, "recipe")
    Q, img = pj.recipe_q(67, 131), field(shape)[3]
    a, b = run_raw(d, Q, img, e), run_raw(d, Q, img, e)
    for k in a:
        if k != "ws":
            assert np.array_equal(a[k], b[k]), k
    big, _ = pattern(BIG, "recipe")
    a, b = run_raw(big, pj.recipe_q(1, BIG[2]), normals=False), run_raw(big, pj.recipe_q(1, BIG[2]), normals=False)
    for k in ("points", "count", "xyz", "index"):
        assert np.array_equal(a[k], b[k]), k


def assert_cloud_is_judge(cloud, d, Q, image=None, exclude=None, what="", **kw):
    """A ``PointCloud`` of the wrapper (rows beyond the count are uninitialised there)."""
    d = np.asarray(d, np.float32)
    d3 = d[None] if d.ndim == 2 else d
    j64 = pj.judge(d3, Q, image=None if image is None else np.asarray(image).reshape(d3.shape + (-1,)),
                   exclude=exclude, **kw)
    j32 = pj.judge(d3, Q, exclude=exclude, dtype=np.float32, **kw)
    count = cloud.count.cpu().numpy().reshape(-1)
    assert np.array_equal(count, j64["count"]), what
    for b in range(d3.shape[0]):
        host = cloud.to_host(b) if d.ndim == 3 else cloud.to_host()
        assert host.count == j64["count"][b] and np.array_equal(host.index, j64["index"][b]), what
        assert image is None or np.array_equal(host.rgb, j64["rgb"][b]), what
        if host.xyz.size:
            assert np.abs(host.xyz.astype(np.float64) - j64["xyz"][b]).max() <= bar(j32["xyz"][b], j64["xyz"][b]), what
        if kw.get("normals"):
            assert np.array_equal((host.normals == 0).all(1), (j64["normals"][b] == 0).all(1)), what
            if host.normals.size:
                assert np.abs(host.normals.astype(np.float64) - j64["normals"][b]).max() <= bar(
                    j32["normals"][b], j64["normals"][b]), what
    return j64


def test_captured_graph_replays_with_a_new_matrix_and_new_data():
    shape = (2, 67, 131)
    d, e = pattern(shape, "recipe")
    img = field(shape)[3]
    Q = pj.recipe_q(67, 131)
    sd, se, si = _dev(d), _dev(e), _dev(img)
    sq = torch.from_numpy(Q.astype(np.float32)).to(DEV)
    run = lambda: kernels.reproject(sd, sq, si, se, normals=True, capacity=8000)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    kw = dict(normals=True, capacity=8000)
    assert_cloud_is_judge(out, d, Q, img, e, "replay", **kw)
    # a new calibration and new maps in the same buffers
    Q2 = pc.q_matrix(650.0, 0.12, 70.0, 30.0, cx_right=68.5, origin=(11, 5))
    d2, e2 = pj.slanted_field(shape, seed=99)
    sq.copy_(torch.from_numpy(Q2.astype(np.float32))), sd.copy_(_dev(d2)), se.copy_(_dev(e2))
    graph.replay()
    j = assert_cloud_is_judge(out, d2, Q2, img, e2, "replay on new values", **kw)
    assert not np.array_equal(j["count"], pj.judge(d, Q, exclude=e)["count"])
    d3, e3 = pattern(shape, "runs64_offset")
    sd.copy_(_dev(d3)), se.copy_(_dev(e3))
    graph.replay()
    assert_cloud_is_judge(out, d3, Q2, img, e3, "replay on the runs", **kw)


def test_wrapper_outputs_views_and_refusals():
    shape = (2, 67, 131)
    d, e = pattern(shape, "recipe")
    img = field(shape)[3]
    Q = pj.recipe_q(67, 131)
    raw = run_raw(d, Q, img, e)
    big = torch.full((2, 134, 133), -3.0, device=DEV)
    big[:, ::2, 1:-1] = _dev(d)
    dv = big[:, ::2, 1:-1]
    assert not dv.is_contiguous()
    cloud = kernels.reproject(dv, torch.from_numpy(Q), _dev(img), _dev(e != 0), normals=True, want_points=True,
                              want_valid=True)
    assert isinstance(cloud, kernels.PointCloud) and cloud._fields == ("points", "valid", "count", "xyz", "rgb", "index",
                                                                         "normals")
    assert np.array_equal(_bits(cloud.points), raw["points"]) and np.array_equal(cloud.valid.cpu().numpy(), raw["valid"])
    for b in range(2):
        host = cloud.to_host(b)
        n = host.count
        assert n == raw["count"][b] and np.array_equal(_bits(host.xyz), raw["xyz"][b, :n])
        assert np.array_equal(host.rgb, raw["rgb"][b, :n]) and np.array_equal(host.index, raw["index"][b, :n])
        assert np.array_equal(_bits(host.normals), raw["normals"][b, :n])
    only = kernels.reproject(_dev(d), Q, want_compact=False, want_valid=True)
    assert only.points is None and only.count is None and only.xyz is None and only.valid is not None
    with pytest.raises(ValueError):
        only.to_host()
    cut = kernels.reproject(_dev(d), Q, exclude=_dev(e), capacity=100)
    assert cut.xyz.shape == (2, 100, 3) and cut.to_host(1).xyz.shape == (100, 3) and cut.to_host(1).count == raw["count"][1]
    with kernels.KernelProbe() as probe:
        kernels.reproject(_dev(d), Q)
    assert probe.summary()["disparity_pointcloud"]["launches"] == 1
    dd = _dev(d)
    for kw in (dict(min_disp=float("nan")), dict(max_disp="1"), dict(normal_max_diff=-1.0), dict(capacity=0),
               dict(capacity=1.5), dict(want_compact=False), dict(normals=True, want_compact=False, want_valid=True),
               dict(exclude=torch.zeros(shape, device=DEV)), dict(exclude=torch.zeros((2, 67, 130), device=DEV, dtype=torch.uint8)),
               dict(image=torch.zeros(shape + (3,), device=DEV)), dict(image=torch.zeros(shape + (2,), device=DEV, dtype=torch.uint8)),
               dict(image=torch.zeros(shape + (3,), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            kernels.reproject(dd, Q, **kw)
    for badq in (np.eye(3), np.zeros((3, 4, 4)), torch.zeros(4, 4, dtype=torch.int32)):
        with pytest.raises(ValueError):
            kernels.reproject(dd, badq)
    for bad in (torch.zeros(6, device=DEV), torch.zeros(1, 1, 6, 7, device=DEV), torch.zeros(0, 6, 7, device=DEV)):
        with pytest.raises(ValueError):
            kernels.reproject(bad, Q)
    with pytest.raises(_lib.HipKernelError):
        kernels.reproject(torch.zeros(1, 6, 7, device=DEV, dtype=torch.float64), Q)
    lib = _lib.load()
    t = torch.zeros(64, device=DEV)
    rc = lib.lea_disparity_pointcloud_f32(t.data_ptr(), None, None, 0, t.data_ptr(), 0, 1, 2, 2, 0.0, 1.0, 1.0, 4,
                                          t.data_ptr() + 128, t.data_ptr(), None, None, None, None, None, None, None)
    assert rc == _lib.LEA_E_INVALID and b"overlaps" in lib.lea_last_error()


# ------------------------------------------------------------------ model level
H, W, MD = 96, 192, 48
REFINE = dict(lam=128.0, sigma=0.1, iterations=2, radius=3, lr_threshold=1.0)
QM = pc.q_matrix(400.0, 0.25, W / 2, H / 2)


@functools.lru_cache(maxsize=None)
def _model():
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def _pair(seed):
    return normal(seed, (1, 3, H, W)).to(DEV), normal(seed + 1, (1, 3, H, W)).to(DEV)


def _same_cloud(a, b):
    """Two PointClouds of the wrapper hold the same bits (up to the count in the compact arrays)."""
    assert torch.equal(a.count, b.count)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
    for bi in range(a.count.numel()):
        ha, hb = a.to_host(bi), b.to_host(bi)
        assert ha.count == hb.count
        for x, y in zip(ha[1:], hb[1:]):
            assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))


def test_forward_points_is_forward_refined_then_reproject():
    m = _model()
    left, right = _pair(11)
    img = _dev(field((1, H, W))[3])
    with torch.no_grad():
        plain = m(left, right)
        ref = m.forward_refined(left, right, **REFINE)
        out, cloud = m.forward_points(left, right, QM, image=img, normals=True, **REFINE)
        raw_out, raw_cloud = m.forward_points(left, right, QM, refine=False, speckle={}, **REFINE)
    assert isinstance(out, kernels.DisparityRefined) and isinstance(cloud, kernels.PointCloud)
    assert torch.equal(out.disp, plain)
    for a, b in zip(out, ref):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    _same_cloud(cloud, kernels.reproject(out.disp_refined, QM, img, out.state, normals=True))
    _same_cloud(raw_cloud, kernels.reproject(raw_out.disp, QM, None, raw_out.state))
    assert torch.equal(raw_out.disp, plain)
    j = assert_cloud_is_judge(cloud, out.disp_refined.cpu().numpy(), QM, img.cpu().numpy(), out.state.cpu().numpy(),
                              "forward_points")
    print(f"forward_points: {int(j['count'][0])} of {H * W} pixels in the cloud, "
          f"{int((out.state != 0).sum())} excluded by the left-right check")
    assert 0 < j["count"][0] < H * W


def test_graphed_points_replays_with_the_matrix_it_holds():
    m = _model()
    g = m.graphed(1, H, W, refine=REFINE, points=dict(Q=QM, normals=True, image=True))
    img = _dev(field((1, H, W))[3])
    Q2 = pc.q_matrix(520.0, 0.4, 90.0, 50.0, origin=(7, 3))
    for seed, Q in ((21, None), (31, Q2)):
        left, right = _pair(seed)
        with torch.no_grad():
            want_out, want = m.forward_points(left, right, QM if Q is None else Q, image=img, normals=True, **REFINE)
        got_out, got = g(left, right, Q=Q, image=img)
        for a, b in zip(got_out, want_out):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        _same_cloud(got, want)
    assert np.array_equal(g.Q.cpu().numpy(), Q2.astype(np.float32))


# ------------------------------------------------------------------ scene level and predict.py
KW = dict(context=8, ramp=8)


def test_points_scene_on_a_two_tile_scene():
    m = _model()
    g = golden("c1_sceneflow")
    left = torch.from_numpy(np.ascontiguousarray(g["left_u8"][:H, :300])).to(DEV)
    right = torch.from_numpy(np.ascontiguousarray(g["right_u8"][:H, :300])).to(DEV)
    runner = scene.SceneRunner(m, H, W, tile_batch=2, confidence=True, radius=3, lr_threshold=1.0, **KW)
    assert len(runner.plan(H, 300)) == 2
    res = runner(left, right)
    Q = pc.q_matrix(400.0, 0.25, 150.0, 48.0)
    cloud = scene.points_scene(res, Q, left, use="disp", normals=True)
    assert cloud.count.shape == () and cloud.xyz.shape == (H * 300, 3)
    _same_cloud(cloud, kernels.reproject(res.disp, Q, left, res.state, normals=True))
    assert_cloud_is_judge(cloud, res.disp.cpu().numpy(), Q, left.cpu().numpy(), res.state.cpu().numpy(), "scene",
                          normals=True)
    _same_cloud(scene.points_scene(res, Q, None, use="filled"), kernels.reproject(res.disp_filled, Q, None, res.state))
    refined = scene.refine_scene(res, left, 128.0, 0.1, 2)
    want = kernels.reproject(refined, Q, left, res.state)
    _same_cloud(scene.points_scene(res, Q, left, use="refined", refined=refined), want)
    _same_cloud(scene.points_scene(res, Q, left, refine=dict(lam=128.0, sigma=0.1, iterations=2)), want)
    with pytest.raises(ValueError):
        scene.points_scene(res, Q, left, use="tiles")
    with pytest.raises(ValueError):
        scene.points_scene(scene.SceneResult(disp=res.disp), Q, None, use="filled")


def test_predict_cli_pointcloud(tmp_path):
    """A 120 x 300 sceneflow-layout pair through a 96 x 192 crop: --pointcloud adds {index}.ply and moves
    nothing else; the cloud is the written map's, without the pixels --lr_check flags, with the
    source image's calibration (the centre crop starts at (54, 12)) and its colours."""
    SH = 120
    from PIL import Image
    from leastereo_amd import predict as P
    g = golden("c1_sceneflow")
    for side in ("left", "right"):
        d = tmp_path / "frames_finalpass" / "S" / side
        d.mkdir(parents=True)
        Image.fromarray(g[side + "_u8"][:SH, :300]).save(d / "0001.png")
    (tmp_path / "list.txt").write_text("S/left/0001.png\n")
    torch.save({"state_dict": {"module." + k: v for k, v in state_dict().items()}}, tmp_path / "ckpt.pth")
    base = ["--sceneflow=1", f"--maxdisp={MD}", "--crop_height=96", "--crop_width=192",
            f"--data_path={tmp_path}/", f"--test_list={tmp_path}/list.txt", f"--resume={tmp_path}/ckpt.pth", "--lr_check=1"]
    assert P.main(base + [f"--save_path={tmp_path}/plain/"]) == 0
    assert P.main(base + [f"--save_path={tmp_path}/cloud/", "--pointcloud=1", "--pc_focal=400", "--pc_baseline=0.25",
                          "--pc_normals=1", "--pc_max_depth=20"]) == 0
    assert sorted(p.name for p in (tmp_path / "cloud").iterdir()) == sorted(
        [p.name for p in (tmp_path / "plain").iterdir()] + ["0.ply"])
    for same in ("0.npy", "0_right.npy", "0_filled.npy"):
        assert np.array_equal(np.load(tmp_path / "plain" / same), np.load(tmp_path / "cloud" / same)), same
    disp = np.load(tmp_path / "cloud" / "0.npy")
    flagged = np.asarray(Image.open(tmp_path / "cloud" / "0_occ.png")) != 0
    assert disp.shape == (H, W) and P.map_origin(SH, 300, H, W) == (54, 12)
    Q = pc.q_matrix(400.0, 0.25, 150.0, 60.0, origin=(54, 12))
    crop = g["left_u8"][12:12 + H, 54:54 + W]
    kw = dict(image=crop[None], exclude=flagged[None].astype(np.uint8), min_disp=np.float32(400.0 * 0.25 / 20.0), normals=True)
    j64, j32 = pj.judge(disp[None], Q, **kw), pj.judge(disp[None], Q, dtype=np.float32, **kw)
    xyz, rgb, nrm = pc.read_ply(tmp_path / "cloud" / "0.ply")
    assert 0 < len(xyz) == j64["count"][0] < H * W and np.array_equal(rgb, j64["rgb"][0])
    assert np.abs(xyz.astype(np.float64) - j64["xyz"][0]).max() <= bar(j32["xyz"][0], j64["xyz"][0])
    assert xyz[:, 2].max() <= 20.0 * (1 + 1e-6)
    assert np.array_equal((nrm == 0).all(1), (j64["normals"][0] == 0).all(1))
    assert np.abs(nrm.astype(np.float64) - j64["normals"][0]).max() <= bar(j32["normals"][0], j64["normals"][0])
    # with --speckle the pixels it removes go too; under --refine 1 the cloud is the refined map's, nothing excluded
    flags = ["--pointcloud=1", "--pc_focal=400", "--pc_baseline=0.25"]
    assert P.main(base + [f"--save_path={tmp_path}/speckle/", "--speckle=60", "--speckle_diff=0.5"] + flags) == 0
    removed = np.asarray(Image.open(tmp_path / "speckle" / "0_speckle.png")) == 255
    print(f"--speckle removes {int(removed.sum())} pixels beside the {int(flagged.sum())} of --lr_check")
    assert not (removed & flagged).any()
    assert P.main(base + [f"--save_path={tmp_path}/refined/", "--refine=1", "--refine_lambda=128", "--refine_sigma=0.1",
                          "--refine_iters=2", "--conf_radius=3"] + flags) == 0
    refined = np.load(tmp_path / "refined" / "0_refined.npy")
    for name, d, ex in (("speckle", disp, (flagged | removed)[None].astype(np.uint8)), ("refined", refined, None)):
        j64, j32 = pj.judge(d[None], Q, exclude=ex), pj.judge(d[None], Q, exclude=ex, dtype=np.float32)
        xyz, rgb, nrm = pc.read_ply(tmp_path / name / "0.ply")
        assert nrm is None and 0 < len(xyz) == j64["count"][0], name
        assert np.array_equal(rgb, crop.reshape(H * W, -1)[j64["index"][0], :3]), name
        assert np.abs(xyz.astype(np.float64) - j64["xyz"][0]).max() <= bar(j32["xyz"][0], j64["xyz"][0]), name
