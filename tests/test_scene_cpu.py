"""Whole-scene inference on the host: the tile planner of leastereo_amd/scene.py against the
origins worked out by hand and against the numpy judge (tests/scene_judge.py), coverage,
the symmetry of the two views' weights, the refusals and the predict flag.  The host-side
AddressSanitizer driver of the two new entries (tests/asan/scene_asan.cpp) runs with its
siblings in tests/test_asan_cpu.py (`make asan`)."""
import os
import subprocess

import numpy as np
import pytest

from leastereo_amd import scene
from tests import scene_judge as J

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(tile_h=96, tile_w=192, maxdisp=48, context=8, ramp=8)
BIG = dict(tile_h=576, tile_w=960, maxdisp=192, context=16, ramp=32)
# (height, width, settings, ys, xs)
CASES = [(150, 300, SMALL, [0, 54], [0, 108]),
         (80, 300, SMALL, [-16], [0, 108]),
         (96, 192, SMALL, [0], [0]),
         (97, 193, SMALL, [0, 1], [0, 1]),
         (300, 700, SMALL, [0, 68, 136, 204], [0, 101, 203, 304, 406, 508]),
         (2048, 2048, BIG, [0, 490, 981, 1472], [0, 544, 1088])]
IDS = [f"{c[0]}x{c[1]}" for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planner_origins(case):
    h, w, kw, ys, xs = case
    p = scene.plan_tiles(h, w, **kw)
    assert (p.ys, p.xs) == (ys, xs)
    assert (p.ny, p.nx, len(p)) == (len(ys), len(xs), len(ys) * len(xs))
    assert p.origins.dtype == np.int32 and p.origins.tolist() == [[y, x] for y in ys for x in xs]
    assert (ys, xs) == tuple(J.plan(h, w, kw["tile_h"], kw["tile_w"], kw["maxdisp"], kw["context"],
                                    kw["ramp"]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planner_covers_and_weights_match_the_judge(case):
    h, w, kw, ys, xs = case
    p = scene.plan_tiles(h, w, **kw)
    assert p.covers()
    for view in ("left", "right"):
        n = p.cover_count(view)
        assert n.min() >= 1 and n.max() <= 4
        print(f"{h}x{w} {view}: {100.0 * float((n == 1).mean()):.1f} % of the pixels have one tile")
        for k in sorted({0, len(p) // 2, len(p) - 1}):
            got = p.weights(k, view)
            want = J.tile_weights(ys, xs, k, h, w, kw["tile_h"], kw["tile_w"], kw["maxdisp"], kw["context"],
                                  kw["ramp"], view)
            assert got.dtype == np.int64 and np.array_equal(got, want)
            assert got.max() <= kw["ramp"] ** 2 <= 65536


def test_guards_are_one_sided():
    p = scene.plan_tiles(150, 300, **SMALL)
    assert p.guards("left") == ((8, 8), (56, 8)) and p.guards("right") == ((8, 8), (8, 56))
    wl, wr = p.weights(3, "left"), p.weights(3, "right")  # the bottom-right tile: cut on top and left
    assert not wl[:8].any() and not wl[:, :56].any() and wl[8, 56] == 1 and wl[-1, -1] == 64
    assert not wr[:, :8].any() and wr[8, 8] == 1 and wr[8, 9] == 2
    # the top-left tile touches the border there: no guard, no ramp
    assert p.weights(0, "left")[0, 0] == 64 and not p.weights(0, "left")[:, -8:].any()
    assert not p.weights(0, "right")[:, -56:].any() and p.weights(0, "right")[0, -57] == 8


def test_random_sizes_cover():
    rng = np.random.default_rng(0)
    for _ in range(20):
        h, w = int(rng.integers(1, 700)), int(rng.integers(1, 1500))
        p = scene.plan_tiles(h, w, **SMALL)
        assert p.covers(), (h, w, p.ys, p.xs)
        assert max(p.cover_count("left").max(), p.cover_count("right").max()) <= 9


@pytest.mark.parametrize("case", CASES[:5], ids=IDS[:5])
def test_views_mirror(case):
    """The right view's x weights are the left view's mirrored, for the mirrored origin list."""
    h, w, kw, ys, xs = case
    p = scene.plan_tiles(h, w, **kw)
    mirrored = scene.TilePlan(h, w, kw["tile_h"], kw["tile_w"], kw["maxdisp"], kw["context"], kw["ramp"], ys,
                              [w - kw["tile_w"] - x for x in reversed(xs)])
    _, wx_right = p.axis_weights("right")
    _, wx_left = mirrored.axis_weights("left")
    assert np.array_equal(wx_right, wx_left[::-1, ::-1])
    wy_left, wy_right = p.axis_weights("left")[0], p.axis_weights("right")[0]
    assert np.array_equal(wy_left, wy_right)


def test_refusals():
    for ramp in (0, -1, 257):
        with pytest.raises(ValueError, match="ramp"):
            scene.plan_tiles(150, 300, 96, 192, 48, context=8, ramp=ramp)
    # y fits the tile; on x the largest stride is 192 - 64 - ramp: 1, then 0
    assert scene.plan_tiles(96, 194, 96, 192, 48, context=8, ramp=127).xs == [0, 1, 2]
    with pytest.raises(ValueError, match="too short"):
        scene.plan_tiles(96, 194, 96, 192, 48, context=8, ramp=128)
    with pytest.raises(ValueError, match="too short"):  # 64 wide: no room for maxdisp + 2 context + ramp
        scene.plan_tiles(150, 300, 96, 64, 48, context=8, ramp=8)
    with pytest.raises(ValueError, match="too short"):
        scene.plan_tiles(150, 300, 24, 192, 48, context=8, ramp=8)
    with pytest.raises(ValueError, match="tiles along"):
        scene.plan_tiles(150, 100000, 96, 192, 48, context=8, ramp=8)
    # a scene that fits the tile needs no room for guards
    assert scene.plan_tiles(20, 60, 24, 64, 48, context=8, ramp=8).origins.tolist() == [[-4, -4]]
    p = scene.plan_tiles(150, 300, **SMALL)
    with pytest.raises(ValueError, match="view"):
        p.guards("up")
    # origins handed in directly: a hole shows
    holed = scene.TilePlan(150, 300, 96, 192, 48, 8, 8, [0, 54], [0])
    assert not holed.covers() and holed.cover_count("left")[:, 192:].max() == 0


def test_runner_batches():
    class Stub:
        maxdisp = 48

        def check_shape(self, h, w):
            assert (h, w) == (96, 192)

    r = scene.SceneRunner(Stub(), 96, 192, tile_batch=3, context=8, ramp=8)
    p = r.plan(150, 300)
    assert p is r.plan(150, 300) and (p.ys, p.xs) == ([0, 54], [0, 108])
    assert r.batches(p) == [[0, 1, 2], [3, -1, -1]]
    assert scene.SceneRunner(Stub(), 96, 192, context=8, ramp=8).batches(p) == [[0], [1], [2], [3]]
    with pytest.raises(ValueError):
        scene.SceneRunner(Stub(), 96, 192, tile_batch=0)
    with pytest.raises(ValueError):
        scene.SceneRunner(Stub(), 96, 192, ramp=300)


def test_predict_flag_parses_and_defaults_off():
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l"]
    opt = obtain_predict_args(base)
    assert (opt.scene, opt.scene_batch, opt.scene_context, opt.scene_ramp) == (0, 1, 16, 32)
    opt = obtain_predict_args(base + ["--scene", "1", "--scene_batch=4", "--scene_context=8", "--scene_ramp=8"])
    assert (opt.scene, opt.scene_batch, opt.scene_context, opt.scene_ramp) == (1, 4, 8, 8)


def test_asan_driver_is_wired_into_make_asan():
    """`make asan` links the driver with every unit and runs it: asked of make itself (a dry run
    of everything), since the drivers are one list and a pattern rule pair in the Makefile."""
    assert os.path.isfile(os.path.join(REPO, "tests", "asan", "scene_asan.cpp"))
    plan = subprocess.run(["make", "-n", "-B", "asan"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert plan.returncode == 0, plan.stderr[-2000:]
    link = [l for l in plan.stdout.splitlines() if " -o build/asan/scene_asan " in l]
    assert len(link) == 1 and "build/asan/scene_asan_main.o" in link[0] and "build/asan/tile_blend.o" in link[0]
    assert "ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/scene_asan" in plan.stdout.splitlines()
