"""The surface model on the GPU (lea_dsm_splat_f32 / lea_dsm_resolve_f32 / lea_dsm_clear,
dsm.Surface, scene.dsm_scene, predict.py --dsm).

Every case compares with tests/dsm_judge.py bit for bit, no cell left out: keys, hits, and after
two fill passes height, rgb or source, and state.  The fields (``dsm_judge.cases``) and what they
are built for are checked without a GPU in tests/test_dsm_cpu.py.

The scatter has two forms.  A workgroup of the LDS-staged form takes 1024 rows and stages the
bounding box of their cells when it has at most 4096 cells: the 65 x 63 grids (4095 cells) and the
one-cell case fit whatever the rows, the 130 x 70 grids (9100 cells, rows all over them) do not,
and the organised 48 x 64 scene fits by patch (``row_width``) as well as by run.
"""
import functools

import numpy as np
import pytest
import torch

from leastereo_amd import dsm, kernels, scene
from leastereo_amd import pointcloud as pc
from tests import dirty_memory as dm
from tests import dsm_judge as J

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = J.cases()
IDS = dict(ids=lambda c: c.name)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)  # a copy: the references are read-only


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def reference(name):
    """The judge's per-item results of a case, computed once, read-only."""
    case = [c for c in CASES if c.name == name][0]
    return J.judge_case(case)


def _surface(case, hits=True):
    return dsm.Surface(case.gh, case.gw, DEV, batch=case.points.shape[0], hits=hits)


def _add(surface, case, **kw):
    return surface.add(_dev(case.points), _dev(case.G), _dev(case.count), _dev(case.colours), radius=case.radius, **kw)


def assert_surface_is_judge(surface, maps, ref, what):
    keys, hits = _u64(surface.keys), surface.hits.cpu().numpy()
    for b, (k, h, _, m, _) in enumerate(ref):
        assert np.array_equal(keys[b], k), f"{what}: keys of item {b}"
        assert np.array_equal(hits[b], h), f"{what}: hits of item {b}"
        if maps is None:
            continue
        assert np.array_equal(_bits(maps.height[b]), m.height.view(np.int32)), f"{what}: height of item {b}"
        assert np.array_equal(maps.state[b].cpu().numpy(), m.state), f"{what}: state of item {b}"
        if maps.rgb is not None:
            assert maps.source is None and np.array_equal(maps.rgb[b].cpu().numpy(), m.rgb), f"{what}: rgb of item {b}"
        else:
            assert np.array_equal(maps.source[b].cpu().numpy(), m.source), f"{what}: source of item {b}"


@pytest.mark.parametrize("case", CASES, **IDS)
@pytest.mark.parametrize("staging", ["global", "lds", "auto"])
def test_bit_for_bit_against_the_judge(case, staging):
    s = _add(_surface(case), case, staging=staging)
    maps = s.resolve(fill_iterations=J.FILL["iterations"], min_neighbours=J.FILL["min_neighbours"])
    assert (maps.rgb is None) == (case.colours is None) and maps.hits is s.hits
    assert_surface_is_judge(s, maps, reference(case.name), f"{case.name} {staging}")
    # resolve works on a copy; a second one gives the same bits; nodata is what was asked for
    assert_surface_is_judge(s, None, reference(case.name), "after resolve")
    again = s.resolve(fill_iterations=J.FILL["iterations"], min_neighbours=J.FILL["min_neighbours"], nodata=-7.5)
    empty = again.state == 2
    assert torch.equal(again.state, maps.state) and bool((again.height[empty] == -7.5).all())
    assert torch.equal(again.height[~empty], maps.height[~empty])
    plain = s.resolve()
    assert bool(((plain.state == 0) == (s.keys != 0)).all()) and not bool((plain.state == 1).any())


@pytest.mark.parametrize("name", ["65x63_r1025_rgb", "130x70_r1025", "65x63_b4_r1500", "one_cell_4096"])
def test_the_forms_and_the_row_width_give_identical_bits(name):
    """Boxes that fit the LDS tile (65 x 63, one cell) and boxes that do not (130 x 70)."""
    case = [c for c in CASES if c.name == name][0]
    rows = case.points.shape[1]
    want = None
    for staging in ("global", "lds", "auto"):
        for width in (0, 41, rows):
            s = _add(_surface(case), case, staging=staging, row_width=width)
            got = (s.keys.clone(), s.hits.clone())
            want = got if want is None else want
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (staging, width)
    assert_surface_is_judge(s, None, reference(name), name)


def test_accumulation_clear_and_identical_calls():
    case = [c for c in CASES if c.name == "65x63_r1025_rgb"][0]
    p, c, G = _dev(case.points), _dev(case.colours), _dev(case.G)
    a, b = slice(0, 400), slice(400, None)
    kw = dict(radius=case.radius)
    grids = []
    for staging in ("global", "lds"):
        whole = dsm.Surface(65, 63, DEV, batch=1, hits=True).add(p, G, colours=c, staging=staging, **kw)
        ab = dsm.Surface(65, 63, DEV, batch=1, hits=True)
        ab.add(p[:, a], G, colours=c[:, a], staging=staging, **kw).add(p[:, b], G, colours=c[:, b], staging=staging, **kw)
        ba = dsm.Surface(65, 63, DEV, batch=1, hits=True)
        ba.add(p[:, b], G, colours=c[:, b], staging=staging, **kw).add(p[:, a], G, colours=c[:, a], staging=staging, **kw)
        grids += [whole, ab, ba]
    for s in grids[1:]:
        assert torch.equal(s.keys, grids[0].keys) and torch.equal(s.hits, grids[0].hits)
    assert_surface_is_judge(grids[0], None, reference(case.name), "whole")
    # two identical calls on a grid that holds them already change nothing but the counts
    s = grids[0]
    before = s.keys.clone()
    s.add(p, G, colours=c, **kw)
    assert torch.equal(s.keys, before) and torch.equal(s.hits, 2 * grids[1].hits)
    # payload kinds do not mix between clears
    with pytest.raises(ValueError, match="mixed"):
        s.add(p, G, **kw)
    s.clear()
    assert not bool(s.keys.any()) and not bool(s.hits.any()) and s.kind is None
    m = s.resolve(fill_iterations=1)
    assert bool((m.state == 2).all()) and bool(torch.isnan(m.height).all()) and bool((m.source == -1).all())
    s.add(p, G, **kw)  # now rows
    assert s.resolve().rgb is None


def test_wrapper_shapes_and_refusals():
    case = [c for c in CASES if c.name == "65x63_r65"][0]
    p, c, G = _dev(case.points[0]), _dev(case.colours[0]), _dev(case.G)
    s = dsm.Surface(65, 63, DEV, hits=True)  # no batch axis
    assert s.keys.shape == (65, 63) and s.keys.dtype == torch.int64 and s.hits.dtype == torch.int32
    maps = s.add(p, G, colours=c, radius=case.radius).resolve(**{"fill_iterations": 2})
    assert maps.height.shape == (65, 63) and maps.rgb.shape == (65, 63, 3)
    k, h, _, m, _ = reference(case.name)[0]
    assert np.array_equal(_u64(s.keys), k) and np.array_equal(s.hits.cpu().numpy(), h)
    assert np.array_equal(_bits(maps.height), m.height.view(np.int32)) and np.array_equal(maps.rgb.cpu().numpy(), m.rgb)
    # a host G is converted; an organised [H, W, 3] block is flattened
    t = dsm.Surface(65, 63, DEV, hits=True).add(p[:64].reshape(8, 8, 3), case.G, colours=c[:64].reshape(8, 8, 3),
                                                 radius=case.radius, row_width=8)
    u = dsm.Surface(65, 63, DEV, hits=True).add(p[:64], case.G, colours=c[:64], radius=case.radius)
    assert torch.equal(t.keys, u.keys) and torch.equal(t.hits, u.hits)
    for bad in (dict(points=p.double()), dict(points=p.cpu()), dict(points=p[:, :2]), dict(points=p[None]),
                dict(G=np.eye(4)), dict(G=torch.eye(3, 4, dtype=torch.int32, device=DEV)),
                dict(colours=c[:10]), dict(colours=c.float()), dict(count=torch.zeros(2, dtype=torch.int32, device=DEV)),
                dict(count=torch.zeros((), dtype=torch.int64, device=DEV)), dict(radius=2.5), dict(radius=-0.1),
                dict(radius=float("nan")), dict(staging="fast"), dict(row_width=-1), dict(row_width=66),
                dict(row_width=1.5)):
        with pytest.raises(ValueError):
            s.add(**dict(dict(points=p, G=G, colours=c), **bad))
    for bad in (dict(fill_iterations=1025), dict(fill_iterations=1.0), dict(min_neighbours=0), dict(nodata="nan")):
        with pytest.raises(ValueError):
            s.resolve(**bad)


def test_captured_graph_replays_with_new_points_and_a_new_matrix():
    a, b = [c for c in CASES if c.name in ("65x63_r1025_rgb", "65x63_r1025_r0")]
    a, b = (a, b) if a.colours is not None else (b, a)
    b_case = b
    p, c, G = _dev(a.points), _dev(a.colours), _dev(a.G)
    s = dsm.Surface(65, 63, DEV, batch=1, hits=True)

    def run():
        s.clear()
        return s.add(p, G, colours=c, radius=2.0, staging="lds").resolve(fill_iterations=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # clear, add, two fill passes, decode: one after the other
        maps = run()
    graph.replay()
    assert_surface_is_judge(s, maps, reference(a.name), "replay")
    # new points, new colours and a new matrix in the same buffers
    G2 = J.rotated_g(65, 63, 5)
    col2 = np.random.default_rng(5).integers(0, 256, b.points.shape, dtype=np.uint8)
    p.copy_(_dev(b.points)), c.copy_(_dev(col2)), G.copy_(_dev(G2))
    graph.replay()
    k, h, _ = J.splat_vec(b.points[0], G2, 65, 63, colours=col2[0], radius=2.0)
    assert not np.array_equal(k, reference(a.name)[0][0])
    assert_surface_is_judge(s, maps, [(k, h, 0, J.resolve(k, **J.FILL), 0)], "replay on new values")
    graph.replay()
    assert_surface_is_judge(s, maps, [(k, h, 0, J.resolve(k, **J.FILL), 0)], "second replay")
    # matrices that hold NaN, infinities, 3e38 and denormals: rows whose u, v or z is not finite are skipped
    for b, G3 in enumerate(J.special_gs()):
        G.copy_(_dev(G3))
        graph.replay()
        k, h, _ = J.splat_vec(b_case.points[0], G3, 65, 63, colours=col2[0], radius=2.0)
        assert_surface_is_judge(s, maps, [(k, h, 0, J.resolve(k, **J.FILL), 0)], f"replay with special matrix {b}")


def test_poisoned_memory():
    """Keys, counts, workspace and outputs from poisoned, guarded allocations: the same bits under
    two poison bytes (and as from clean memory), the guards intact."""
    case = [c for c in CASES if c.name == "65x63_b4_r1500"][0]
    p, c, G, n = _dev(case.points), _dev(case.colours), _dev(case.G), _dev(case.count)
    got = {}
    for byte in (dm.NAN, dm.BIG):
        for staging in ("global", "lds"):
            with dm.dirty(byte, DEV) as mem:
                s = dsm.Surface(case.gh, case.gw, DEV, batch=4, hits=True)
                maps = s.add(p, G, n, c, radius=case.radius, staging=staging).resolve(fill_iterations=2)
                torch.cuda.synchronize()
                mem.check()
                assert len(mem.allocations) == 6  # keys, hits, workspace, height, state, rgb
            got[byte, staging] = [dm.bits(t) for t in (s.keys, s.hits, maps.height, maps.rgb, maps.state)]
            assert_surface_is_judge(s, maps, reference(case.name), f"0x{byte:02X} {staging}")
    first = got[dm.NAN, "global"]
    for key, tensors in got.items():
        for x, y in zip(tensors, first):
            assert torch.equal(x, y), key


# ------------------------------------------------------------------ geometry end to end

def test_layered_scene_end_to_end():
    """reproject -> add_cloud -> resolve on a ground plane with a box, against the float64 judge."""
    d, Q, G64, gh, gw, roof = J.layered_scene()
    G = G64.astype(np.float32)
    h, w = d.shape[1:]
    cloud = kernels.reproject(_dev(d), Q, want_points=True)
    assert cloud.count.cpu().tolist() == [h * w, h * w]
    both = cloud.xyz.reshape(1, 2 * h * w, 3)  # item 0's rows, then item 1's: the rows of the judges
    s = dsm.Surface(gh, gw, DEV, batch=1, hits=True).add(both, G, radius=J.SCENE["radius"])
    maps = s.resolve()
    m, h64, s64, agree = J.scene_judges(both[0].cpu().numpy(), d, Q, G64, gh, gw)
    assert np.array_equal(_u64(s.keys[0]), J.splat_vec(both[0].cpu().numpy(), G, gh, gw, radius=J.SCENE["radius"])[0])
    assert np.array_equal(maps.source[0].cpu().numpy(), m.source)
    hit = m.source >= 0
    assert int((hit & ~agree).sum()) <= 0.01 * int(hit.sum())
    got = maps.height[0].cpu().numpy().astype(np.float64)
    e32 = float(np.abs(m.height.astype(np.float64) - h64)[agree].max())
    err = float(np.abs(got - h64)[agree].max())
    bar = max(4.0 * e32, 8.0 * float(np.spacing(np.float32(np.abs(h64[agree]).max()))))
    print(f"layered scene: error {err:.3e}, float32 restatement {e32:.3e}, bar {bar:.3e}, ratio to the restatement "
          f"{err / e32 if e32 else float('nan'):.2f}, {int((hit & ~agree).sum())} of {int(hit.sum())} cells left out")
    assert err <= bar
    # the z-test: the roof's cells carry the roof, though the bare ground lies under them
    top = maps.height[0].cpu().numpy()[roof]
    assert top.size >= 100 and np.all(np.abs(top + J.SCENE["z_roof"]) < 1e-4)
    # the same mosaic cloud by cloud, in either order, through the PointCloud route
    one = lambda b: kernels.PointCloud(None, None, cloud.count[b], cloud.xyz[b], None, None, None)  # noqa: E731
    for order in ((0, 1), (1, 0)):
        t = dsm.Surface(gh, gw, DEV)
        for b in order:
            t.add_cloud(one(b), G, radius=J.SCENE["radius"])
        assert torch.equal(dm.bits(t.resolve().height), dm.bits(maps.height[0])), order
    # the organised points (patches of the image through row_width) give the same grid as the compact rows
    org = kernels.PointCloud(cloud.points[0], None, None, None, None, None, None)
    for staging in ("global", "lds"):
        t = dsm.Surface(gh, gw, DEV).add_cloud(org, G, radius=J.SCENE["radius"], staging=staging)
        u = dsm.Surface(gh, gw, DEV).add_cloud(one(0), G, radius=J.SCENE["radius"], staging=staging)
        assert torch.equal(t.keys, u.keys), staging


H, W, MD = 96, 192, 48


@functools.lru_cache(maxsize=None)
def _model():
    from leastereo_amd.config import LEAStereoArgs, default_arch_args
    from leastereo_amd.model import LEAStereo
    from tests.golden_util import state_dict
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def test_dsm_scene_on_a_one_tile_scene():
    from tests.golden_util import golden
    g = golden("c1_sceneflow")
    left = torch.from_numpy(np.ascontiguousarray(g["left_u8"][:H, :W])).to(DEV)
    right = torch.from_numpy(np.ascontiguousarray(g["right_u8"][:H, :W])).to(DEV)
    runner = scene.SceneRunner(_model(), H, W, tile_batch=1, lr_threshold=1.0, context=8, ramp=8)
    assert len(runner.plan(H, W)) == 1
    res = runner(left, right)
    Q = pc.q_matrix(400.0, 0.25, W / 2, H / 2)
    grid = dsm.grid_from_view(Q, H, W, (2.0, float(MD)), cell=0.05)
    maps = scene.dsm_scene(res, Q, left, grid=grid, radius=0.5, use="disp", fill_iterations=1)
    G, gh, gw = grid
    cloud = kernels.reproject(res.disp, Q, left, res.state)
    want = dsm.Surface(gh, gw, DEV).add_cloud(cloud, G, radius=0.5).resolve(fill_iterations=1)
    assert maps.height.shape == (gh, gw) and bool((maps.state == 0).any())
    for x, y in zip(maps[:4], want[:4]):
        assert (x is None and y is None) or torch.equal(dm.bits(x), dm.bits(y))
    same = scene.dsm_scene(res, Q, left, cell=0.05, disp_range=(2.0, float(MD)), use="disp", fill_iterations=1)
    assert torch.equal(dm.bits(same.height), dm.bits(want.height))
    with pytest.raises(ValueError, match="disp_range"):
        scene.dsm_scene(res, Q, left, use="disp")


def test_predict_cli_dsm(tmp_path):
    """--dsm adds its five files, of one grid, and moves nothing else."""
    import json

    from PIL import Image

    from leastereo_amd import predict as P
    from tests.golden_util import golden, state_dict
    g = golden("c1_sceneflow")
    for side in ("left", "right"):
        d = tmp_path / "frames_finalpass" / "S" / side
        d.mkdir(parents=True)
        Image.fromarray(g[side + "_u8"][:H, :W]).save(d / "0001.png")
    (tmp_path / "list.txt").write_text("S/left/0001.png\n")
    torch.save({"state_dict": {"module." + k: v for k, v in state_dict().items()}}, tmp_path / "ckpt.pth")
    base = ["--sceneflow=1", f"--maxdisp={MD}", f"--crop_height={H}", f"--crop_width={W}",
            f"--data_path={tmp_path}/", f"--test_list={tmp_path}/list.txt", f"--resume={tmp_path}/ckpt.pth"]
    assert P.main(base + [f"--save_path={tmp_path}/plain/"]) == 0
    assert P.main(base + [f"--save_path={tmp_path}/dsm/", "--dsm=1", "--pc_focal=400", "--pc_baseline=0.25",
                          "--pc_max_depth=50", "--dsm_cell=0.05", "--dsm_fill=2"]) == 0
    new = ["0_dsm.npy", "0_dsm.png", "0_ortho.png", "0_dsm_state.png", "0_dsm.json"]
    assert sorted(p.name for p in (tmp_path / "dsm").iterdir()) == sorted(
        [p.name for p in (tmp_path / "plain").iterdir()] + new)
    assert np.array_equal(np.load(tmp_path / "plain" / "0.npy"), np.load(tmp_path / "dsm" / "0.npy"))
    meta = json.loads((tmp_path / "dsm" / "0_dsm.json").read_text())
    gh, gw = meta["size"]
    height = np.load(tmp_path / "dsm" / "0_dsm.npy")
    assert height.dtype == np.float32 and height.shape == (gh, gw) and np.isfinite(height).any()
    assert abs(meta["cell"] - 0.05) < 1e-6 and np.array(meta["G"]).shape == (3, 4) and len(meta["origin"]) == 3
    assert np.asarray(Image.open(tmp_path / "dsm" / "0_dsm.png")).shape[:2] == (gh, gw)
    assert np.asarray(Image.open(tmp_path / "dsm" / "0_ortho.png")).shape == (gh, gw, 3)
    state = np.asarray(Image.open(tmp_path / "dsm" / "0_dsm_state.png"))
    assert state.shape == (gh, gw) and set(np.unique(state)) <= {0, 127, 255}
    assert np.array_equal(state == 255, np.isnan(height))
    # the heights are minus the depths of the map's points
    disp = np.load(tmp_path / "dsm" / "0.npy")
    depth = 400.0 * 0.25 / disp[np.isfinite(disp) & (disp > 2.0)]
    assert -depth.max() - 1e-3 <= np.nanmin(height) and np.nanmax(height) <= -depth.min() + 1e-3
