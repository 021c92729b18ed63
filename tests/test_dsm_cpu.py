"""The surface model without a GPU: the numpy judge against itself and against hand-made grids,
the key's order, the host geometry of ``leastereo_amd.dsm``, the wrapper's refusals, the binding
and predict.py's flags."""
import ctypes

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, dsm
from tests import dsm_judge as J

F = np.float32
U64 = np.uint64


def _key(z, payload):
    return (int(J.ord32(np.array([z], F).view(np.uint32))[0]) << 32) | int(payload)


# ---- the judge

@pytest.mark.parametrize("case", J.cases(), ids=lambda c: c.name)
def test_the_two_forms_of_the_judge_agree(case):
    vec, loop = J.judge_case(case, J.splat_vec), J.judge_case(case, J.splat_loop)
    for (k0, h0, s0, m0, n0), (k1, h1, s1, m1, n1) in zip(vec, loop):
        assert np.array_equal(k0, k1) and np.array_equal(h0, h1) and s0 == s1 and n0 == n1
        assert np.array_equal(m0.keys, m1.keys)


def test_the_fields_meet_their_conditions():
    """What the GPU cases are built for: empty cells, cells under several rows, cells the fill
    passes fill, skipped rows."""
    seen = 0
    for case in J.cases():
        if not case.conditions:
            continue
        seen += 1
        res = J.judge_case(case)
        cells = len(res) * case.gh * case.gw
        read = sum(r[4] for r in res)
        assert sum(int((r[0] == 0).sum()) for r in res) >= 0.05 * cells, case.name
        assert int((J.cover_counts(case) >= 2).sum()) >= 0.05 * cells, case.name
        assert sum(int((r[3].state == 1).sum()) for r in res) >= 0.01 * cells, case.name
        assert sum(r[2] for r in res) >= 0.01 * read, case.name
    assert seen >= 4
    batch = [c for c in J.cases() if c.count is not None][0]
    assert batch.count[0] == 0 and 0 < batch.count[1] < batch.points.shape[1] < batch.count[2]
    assert len({batch.G[b].tobytes() for b in range(1, 4)}) == 3


def test_the_special_matrices_reach_every_skip_test():
    """The case with NaN, infinities, +-1e30, 3e38 and denormals in G: with finite points, u, v or
    z is not finite for at least 1 % of the rows of items 0 .. 4 (all rows of items 0 and 4, a part
    of items 2 and 3: the kernel's second test is what answers for them), item 1 is decided by the
    2^30 test, item 5 skips the rows the plain matrix skips, and the sum of item 2 overflows where
    neither product does."""
    case = [c for c in J.cases() if c.name == "65x63_b6_special_g"][0]
    G, rows = case.G, case.points.shape[1]
    assert G.shape == (6, 3, 4) and np.isnan(G).any() and np.isposinf(G).any() and np.isneginf(G).any()
    assert (np.abs(G) == F(1e30)).any() and (np.abs(G) == F(3e38)).any()
    assert ((G != 0) & (np.abs(G) < np.finfo(F).tiny)).any()
    reasons = [J.skip_reasons(case.points[b], G[b]) for b in range(6)]
    res = J.judge_case(case)
    for b, ((bad_p, bad_uvz, far), r) in enumerate(zip(reasons, res)):
        assert bad_p >= 10 and r[2] == bad_p + bad_uvz + far, b
        assert r[2] >= 0.01 * rows, b
    assert reasons[0][1] == rows - reasons[0][0] and not (res[0][0] != 0).any()
    assert reasons[4][1] == rows - reasons[4][0] and not (res[4][0] != 0).any()
    assert reasons[1][2] >= 0.5 * rows and (res[1][0] != 0).any()
    for b in (2, 3):
        assert 0.01 * rows <= reasons[b][1] < rows - reasons[b][0] and (res[b][0] != 0).any(), b
    assert reasons[5][1] == 0 and reasons[5] == J.skip_reasons(case.points[5], J.AXIS_G)  # the planted huge coordinates alone
    # item 2: the rows the sum loses have two finite terms
    p = case.points[2]
    with np.errstate(all="ignore"):
        prod, off = G[2, 2, 2] * p[:, 2], G[2, 2, 3]
        lost = np.isfinite(p).all(1) & np.isfinite(prod) & ~np.isfinite(prod + off)
    assert 0.01 * rows <= int(lost.sum()) <= reasons[2][1]  # the rest: planted heights whose product overflows
    # heights near FLT_MAX are heights like any other
    assert float(res[2][3].height[res[2][0] != 0].max()) > 3e38


def test_accumulation_is_order_independent_in_the_judge():
    case = [c for c in J.cases() if c.name == "65x63_r1025_r0"][0]
    p = case.points[0]
    a, b = p[:500], p[500:]
    # the source payload is the row of the call, so each half keeps rows of its own: colours instead
    col = np.random.default_rng(0).integers(0, 256, (p.shape[0], 3), dtype=np.uint8)
    whole = J.splat_vec(p, case.G, 65, 63, colours=col)
    ab = J.splat_vec(b, case.G, 65, 63, colours=col[500:], keys=J.splat_vec(a, case.G, 65, 63, colours=col[:500])[0])
    ba = J.splat_vec(a, case.G, 65, 63, colours=col[:500], keys=J.splat_vec(b, case.G, 65, 63, colours=col[500:])[0])
    assert np.array_equal(whole[0], ab[0]) and np.array_equal(whole[0], ba[0])


# ---- the key

def test_ord_is_strictly_monotone_and_round_trips():
    fmax, tiny, dmax = np.finfo(F).max, F(1e-45), np.nextafter(np.finfo(F).tiny, F(0))
    z = np.array([-fmax, -1e30, -1.0, -np.finfo(F).tiny, -dmax, -tiny, -0.0, 0.0, tiny, dmax, np.finfo(F).tiny, 1.0,
                  1e30, fmax], F)
    assert tiny > 0 and dmax < np.finfo(F).tiny  # denormals, kept as such
    o = J.ord32(z.view(np.uint32))
    assert o.dtype == np.uint32 and np.all(o[1:] > o[:-1])
    assert int(o.min()) >= 0x00800000  # a hit is never the empty key
    assert np.array_equal(J.unord32(o), z.view(np.uint32))
    assert [J._ord_int(float(v)) for v in z] == [int(v) for v in o]
    rnd = np.random.default_rng(1).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    rnd = rnd[np.isfinite(rnd.view(F))]
    assert np.array_equal(J.unord32(J.ord32(rnd)), rnd)
    order = np.argsort(rnd.view(F), kind="stable")
    zs, os_ = rnd.view(F)[order], J.ord32(rnd)[order].astype(np.int64)
    assert np.all(np.diff(os_)[np.diff(zs) > 0] > 0)


# ---- the footprint

def test_footprint_spans():
    def cells(u, radius, n=10):
        lo, hi, near = J.span(np.array([u], F), radius, n)
        return int(lo[0]), int(hi[0]), int(near[0])
    assert cells(3.2, 0.0) == (3, 3, 3)
    assert cells(3.5, 0.0) == (4, 4, 4)  # exactly on i + 0.5: the upper cell
    assert cells(3.499999, 0.0) == (3, 3, 3)
    assert cells(-0.5, 0.0) == (0, 0, 0) and cells(np.nextafter(F(-0.5), F(-1)), 0.0) == (0, -1, -1)  # empty: clipped away
    assert cells(9.5, 0.0) == (10, 9, 10)  # GW - 0.5 is outside
    assert cells(3.2, 0.5) == (3, 4, 3)  # floor((3.2 - 0.5) + 0.5) .. floor((3.2 + 0.5) + 0.5)
    assert cells(3.25, 0.5) == (3, 4, 3)
    assert cells(3.5, 0.5) == (3, 4, 4)
    assert cells(3.75, 0.5) == (3, 4, 4)
    assert cells(4.0, 0.5) == (4, 5, 4)
    assert cells(3.2, 2.0) == (1, 5, 3)
    assert cells(3.5, 2.0) == (2, 6, 4)
    assert cells(0.2, 2.0) == (0, 2, 0) and cells(8.7, 2.0) == (7, 9, 9)  # clipped
    assert cells(-2.6, 2.0) == (0, -1, -3) and cells(-2.5, 2.0) == (0, 0, -2)
    # at most 5 cells an axis
    t = np.random.default_rng(2).uniform(-5, 15, 2000).astype(F)
    lo, hi, _ = J.span(t, 2.0, 1000000)
    assert int((hi - lo).max()) == 4


# ---- the fill rule

def _grid(cells):
    g = np.zeros((5, 5), U64)
    for (y, x), k in cells.items():
        g[y, x] = k
    return g


def test_fill_rule_on_hand_made_grids():
    a, b, c = _key(1.0, 7), _key(2.0, 3), _key(-4.0, 9)
    g = _grid({(0, 0): a, (0, 1): b, (1, 0): c})
    # (1, 1) has three neighbours: the lowest surface, c
    out = J.fill_pass(g, 3)
    want = g.copy()
    want[1, 1] = c
    assert np.array_equal(out, want)
    # min_neighbours 1: every cell beside a hit; (0, 2) and (1, 2) see b alone, (2, 0) and (2, 1) see c
    out = J.fill_pass(g, 1)
    want = g.copy()
    want[1, 1], want[0, 2], want[1, 2], want[2, 0], want[2, 1] = c, b, b, c, c
    assert np.array_equal(out, want)
    # min_neighbours 8: only a cell with all eight neighbours, so none at an edge
    ring = _grid({(y, x): _key(float(y + x), y) for y in range(1, 4) for x in range(1, 4) if (y, x) != (2, 2)})
    out = J.fill_pass(ring, 8)
    want = ring.copy()
    want[2, 2] = _key(2.0, 1)  # the lowest is (1, 1) at height 2, payload 1
    assert np.array_equal(out, want)
    edge = _grid({(y, x): a for y in range(0, 2) for x in range(0, 3) if (y, x) != (0, 1)})
    assert np.array_equal(J.fill_pass(edge, 8), edge)
    # two passes: the second reads what the first wrote, not more
    line = _grid({(2, 0): a, (1, 0): a, (3, 0): a})
    one, two = J.fill_pass(line, 2), J.fill_pass(J.fill_pass(line, 2), 2)
    assert int((one != 0).sum()) == 6 and set(zip(*np.nonzero(one))) == {(1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (3, 1)}
    assert set(zip(*np.nonzero(two))) == {(y, x) for y in range(0, 5) for x in range(0, 3)} - {(0, 2), (4, 2)}
    m = J.resolve(line, 2, 2, nodata=-9.0)
    assert np.array_equal(m.keys, two)
    assert m.state[2, 0] == 0 and m.state[2, 1] == 1 and m.state[2, 4] == 2
    assert m.height[2, 4] == F(-9.0) and m.height[2, 1] == F(1.0) and m.source[2, 4] == -1
    # a tie in height: the smaller payload is the smaller key
    tie = _grid({(0, 0): _key(5.0, 200), (0, 1): _key(5.0, 100), (1, 0): _key(6.0, 1)})
    assert J.fill_pass(tie, 3)[1, 1] == _key(5.0, 100)
    # the surface's own keys are not changed
    assert np.array_equal(line, _grid({(2, 0): a, (1, 0): a, (3, 0): a}))


def test_decode():
    k = _grid({(0, 0): (_key(-0.0, 0x0A0B0C)), (0, 1): _key(3.5, J.FULL - 41)})
    m = J.resolve(k)
    assert m.height[0, 0].view(np.uint32) == 0x80000000 and tuple(m.rgb[0, 0]) == (10, 11, 12)
    assert m.height[0, 1] == F(3.5) and m.source[0, 1] == 41
    assert np.isnan(m.height[1, 1]) and tuple(m.rgb[1, 1]) == (0, 0, 0) and m.state[1, 1] == 2


# ---- the host geometry

def test_grid_matrix_nadir():
    G = dsm.grid_matrix((-4.0, -3.0, 0.0), 0.125, z0=100.0)
    assert G.dtype == np.float32 and G.shape == (3, 4)
    want = np.array([[8, 0, 0, 32], [0, 8, 0, 24], [0, 0, -1, 100]], np.float64)
    assert np.array_equal(G.astype(np.float64), want)
    # height is z0 - Z; the cell centres are integers
    u, v, z = J.project64(np.array([[-4.0, -3.0, 7.0], [-3.875, -2.75, 9.0]]), G)
    assert np.array_equal(u, [0, 1]) and np.array_equal(v, [0, 2]) and np.array_equal(z, [93, 91])


def test_grid_matrix_rotated_30_degrees():
    a = np.deg2rad(30.0)
    c, s = np.cos(a), np.sin(a)
    pose = np.eye(4)
    pose[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]  # the rig turned about its optical axis
    pose[:3, 3] = (10.0, 20.0, 500.0)
    origin, cell = (2.0, 4.0, 100.0), 0.5
    G64 = dsm.grid_matrix64(origin, cell, pose=pose)
    want = np.array([[c / cell, -s / cell, 0, (10.0 - 2.0) / cell],
                     [s / cell, c / cell, 0, (20.0 - 4.0) / cell],
                     [0, 0, -1, -(500.0 - 100.0)]])
    assert np.allclose(G64, want, rtol=0, atol=1e-12)
    G = dsm.grid_matrix(origin, cell, pose=pose)
    assert np.allclose(G, want, rtol=2.0 ** -23, atol=0)
    assert np.array_equal(G, G64.astype(np.float32))  # rounded once
    # other axes: a grid whose rows run along world -y, heights along +z
    G2 = dsm.grid_matrix64((0, 0, 0), 2.0, v_axis=(0, -1, 0), z_axis=(0, 0, 1), z0=1.5)
    assert np.array_equal(G2, [[0.5, 0, 0, 0], [0, -0.5, 0, 0], [0, 0, 1, 1.5]])
    for bad in (dict(cell=0.0), dict(cell=np.nan), dict(pose=np.eye(3)), dict(z0=np.inf)):
        with pytest.raises(ValueError):
            dsm.grid_matrix(**dict(dict(origin=(0, 0, 0), cell=1.0), **bad))
    with pytest.raises(ValueError):
        dsm.grid_matrix((0, 0), 1.0)


def test_grid_from_view():
    from leastereo_amd.pointcloud import q_matrix
    f, base, h, w = 100.0, 0.5, 11, 21
    Q = q_matrix(f, base, 10.0, 5.0)
    # far: d = 5, Z = 10, X in -1 .. 1, Y in -0.5 .. 0.5; near: d = 10, Z = 5, inside that
    G, gh, gw = dsm.grid_from_view(Q, h, w, (5.0, 10.0))
    cell = 10.0 / f  # the ground sample distance at the far disparity
    assert (gh, gw) == (11, 21)
    want = np.array([[1 / cell, 0, 0, 1.0 / cell], [0, 1 / cell, 0, 0.5 / cell], [0, 0, -1, 0]])
    assert np.allclose(G, want, rtol=2.0 ** -22, atol=1e-6) and G.dtype == np.float32
    assert dsm.grid_from_view(Q, h, w, (10.0, 5.0))[1:] == (11, 21)  # the order of the two does not matter
    G2, gh2, gw2 = dsm.grid_from_view(Q, h, w, (5.0, 10.0), cell=0.25)
    assert (gh2, gw2) == (5, 9) and np.allclose(G2[0], [4, 0, 0, 4], atol=1e-6)
    # the rig turned by 30 degrees about its optical axis: the bounding box of the turned rectangle
    a = np.deg2rad(30.0)
    c, s = np.cos(a), np.sin(a)
    pose = np.eye(4)
    pose[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    G3, gh3, gw3 = dsm.grid_from_view(Q, h, w, (5.0, 10.0), cell=0.1, pose=pose)
    wx, wy = 2 * (1.0 * c + 0.5 * s), 2 * (1.0 * s + 0.5 * c)
    assert (gh3, gw3) == (int(np.floor(wy / 0.1 + 0.5)) + 1, int(np.floor(wx / 0.1 + 0.5)) + 1)
    assert np.allclose(G3[0], [c / 0.1, -s / 0.1, 0, (wx / 2) / 0.1], rtol=1e-6, atol=1e-5)
    assert np.allclose(G3[1], [s / 0.1, c / 0.1, 0, (wy / 2) / 0.1], rtol=1e-6, atol=1e-5)
    for bad in ((5.0, 5.0), (np.nan, 1.0), (1.0,)):
        with pytest.raises(ValueError):
            dsm.grid_from_view(Q, h, w, bad)
    with pytest.raises(ValueError):
        dsm.grid_from_view(Q, h, w, (0.0, 5.0))  # disparity 0 is at infinity
    with pytest.raises(ValueError):
        dsm.grid_from_view(Q[:3], h, w, (5.0, 10.0))


# ---- the wrapper, the binding, the flags

def test_wrapper_refusals_that_need_no_library():
    for bad in (dict(gh=0), dict(gw=-1), dict(gh=1.5), dict(batch=0), dict(batch=65536), dict(gh=1 << 16, gw=1 << 15)):
        with pytest.raises(ValueError):
            dsm.Surface(**dict(dict(gh=4, gw=4, device="cuda"), **bad))
    with pytest.raises(_lib.HipKernelError):
        dsm.Surface(4, 4, "cpu")
    s = object.__new__(dsm.Surface)  # the checks of add come before any launch
    s.gh, s.gw, s.b, s.batch, s.device, s.kind = 4, 4, 1, None, torch.device("cpu"), None
    with pytest.raises(ValueError, match="points"):
        s.add(torch.zeros(5, 3), np.eye(3, 4))
    with pytest.raises(ValueError, match="points"):
        s.add(np.zeros((5, 3), F), np.eye(3, 4))
    with pytest.raises(ValueError, match="add_cloud"):
        s.add_cloud("cloud", np.eye(3, 4))
    with pytest.raises(ValueError, match="fill_iterations"):
        s.resolve(fill_iterations=-1)
    with pytest.raises(ValueError, match="min_neighbours"):
        s.resolve(min_neighbours=9)
    with pytest.raises(ValueError, match="min_neighbours"):
        s.resolve(min_neighbours=0)
    assert dsm.STAGING == {"auto": 0, "global": 1, "lds": 2} and dsm.MAX_RADIUS == 2


def test_signatures():
    launches = {n for n, (res, args) in _lib.SIGNATURES.items()
                if res is ctypes.c_int and args and args[-1] is ctypes.c_void_p}
    lib = _lib.load()
    for name, nargs in (("lea_dsm_splat_f32", 15), ("lea_dsm_resolve_f32", 14), ("lea_dsm_clear", 6)):
        assert name in launches and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["lea_dsm_resolve_workspace_bytes"][0] is ctypes.c_size_t
    assert "lea_dsm_resolve_workspace_bytes" not in launches
    assert _lib.SIGNATURES["lea_dsm_splat_f32"][1][4] is ctypes.c_int64  # G's batch stride
    assert _lib.SIGNATURES["lea_dsm_splat_f32"][1][8] is ctypes.c_float  # radius
    assert lib.lea_dsm_resolve_workspace_bytes(2, 5, 6) == 960 and lib.lea_dsm_resolve_workspace_bytes(0, 5, 6) == 0
    assert lib.lea_abi_version() == 14
    # refused before any launch (no device here)
    x = ctypes.c_void_p(64)
    assert lib.lea_dsm_splat_f32(None, None, None, x, 0, 1, 1, 0, 0.0, 0, 1, 1, x, None, None) == _lib.LEA_E_INVALID
    assert b"lea_dsm_splat_f32" in lib.lea_last_error()
    assert lib.lea_dsm_splat_f32(x, None, None, ctypes.c_void_p(1024), 0, 1, 1, 0, 2.5, 0, 1, 1, ctypes.c_void_p(4096),
                                 None, None) == _lib.LEA_E_INVALID
    assert b"radius" in lib.lea_last_error()
    assert lib.lea_dsm_resolve_f32(x, None, 1, 1, 1, 0, 3, 0.0, None, None, None, None, None, None) == _lib.LEA_E_INVALID
    assert lib.lea_dsm_clear(None, None, 1, 1, 1, None) == _lib.LEA_E_INVALID


def test_predict_flags():
    from leastereo_amd import predict
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt"]
    cal = ["--pc_focal=400", "--pc_baseline=0.25"]
    assert predict.dsm_options(obtain_predict_args(base)) is None
    assert predict.dsm_options(obtain_predict_args(base + ["--dsm_cell=-1", "--dsm_radius=9"])) is None  # off
    got = predict.dsm_options(obtain_predict_args(base + cal + ["--dsm=1"]))
    assert got == dict(calib=dict(focal=400.0, baseline=0.25, cx=None, cy=None, max_depth=0.0, normals=False),
                       cell=None, radius=0.5, fill=0)
    got = predict.dsm_options(obtain_predict_args(base + cal + ["--dsm=1", "--dsm_cell=0.05", "--dsm_radius=0",
                                                                "--dsm_fill=3", "--pc_max_depth=40"]))
    assert (got["cell"], got["radius"], got["fill"], got["calib"]["max_depth"]) == (0.05, 0.0, 3, 40.0)
    got = predict.dsm_options(obtain_predict_args(base + ["--dsm=1", "--calib=rig.json"]))
    assert got["calib"]["focal"] is None  # main takes it from the rectification
    # without the flag nothing changes
    old, new = vars(obtain_predict_args(base + cal)), vars(obtain_predict_args(base + cal + ["--dsm=1"]))
    assert {k for k in new if new[k] != old.get(k, None)} == {"dsm"}
    assert predict.pointcloud_options(obtain_predict_args(base + cal + ["--dsm=1"])) is None
    with pytest.raises(ValueError, match="--dsm needs the calibration"):
        predict.dsm_options(obtain_predict_args(base + ["--dsm=1"]))
    with pytest.raises(ValueError, match="--dsm needs the calibration"):
        predict.dsm_options(obtain_predict_args(base + ["--dsm=1", "--pc_focal=400"]))
    with pytest.raises(ValueError, match="--dsm needs the calibration"):
        predict.dsm_options(obtain_predict_args(base + cal + ["--dsm=1", "--calib=rig.json"]))
    for bad in ("--dsm_cell=-0.5", "--dsm_cell=nan", "--dsm_cell=inf", "--dsm_radius=2.5", "--dsm_radius=-1",
                "--dsm_radius=nan", "--dsm_fill=-1", "--dsm_fill=2000"):
        with pytest.raises(ValueError, match=bad.split("=")[0]):
            predict.dsm_options(obtain_predict_args(base + cal + ["--dsm=1", bad]))
    with pytest.raises(NotImplementedError, match="--dsm"):
        predict.dsm_options(obtain_predict_args(base + cal + ["--dsm=1", "--satellite=1"]))
    # main refuses before it needs a device
    with pytest.raises(ValueError, match="--dsm"):
        predict.main(base + ["--sceneflow=1", "--dsm=1"])


def test_the_layered_scene_suits_the_geometry_test():
    """The judge alone on the scene of the GPU's end-to-end test: the float32 and the float64
    geometry disagree on at most 1 % of the hit cells, and the roof's cells carry the roof."""
    from tests import pointcloud_judge as pj
    d, Q, G64, gh, gw, roof = J.layered_scene()
    p32 = pj.reproject_all(d, Q, dtype=np.float32)[0].reshape(-1, 3)
    m, h64, s64, agree = J.scene_judges(p32, d, Q, G64, gh, gw)
    hit = m.source >= 0
    assert np.array_equal(hit, s64 >= 0) and hit.sum() > 3000
    assert int((hit & ~agree).sum()) <= 0.01 * int(hit.sum())
    assert m.height[roof].size >= 100 and np.all(np.abs(m.height[roof] + F(J.SCENE["z_roof"])) < 1e-4)
    # the ground alone would put its own height there
    ground = J.resolve(J.splat_vec(p32[d[0].size:], G64.astype(F), gh, gw, radius=J.SCENE["radius"])[0])
    assert np.all(np.abs(ground.height[roof] + F(J.SCENE["z_ground"])) < 1e-4)
