"""The speckle filter without a GPU: the two forms of the judge (tests/speckle_judge.py) agree
on every input recipe of tests/test_gpu_speckle.py, hand-checked cases pin each rule of the
definition, the C entries refuse what the header says they refuse (fake device addresses: the
checks compare them and never dereference), and the Python layers above make no speckle call
unless they are asked to."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels
from tests import speckle_judge as sj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lea_disparity_speckle_workspace_bytes", "lea_disparity_speckle_f32")
INVALID = _lib.LEA_E_INVALID
P = ctypes.c_void_p

RANDOM_SHAPES = [(1, 1, 1), (1, 1, 257), (1, 33, 1), (2, 67, 131), (1, 130, 70), (1, 33, 129)]
STRUCTURES = [("serpentine", sj.serpentine, 1.0), ("spiral", sj.spiral, 1.0), ("comb", sj.comb, 1.0),
              ("checkerboard", sj.checkerboard, 0.0), ("constant", sj.constant_pair, 1.0)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("max_diff", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_judge_forms_agree_on_the_random_fields(shape, max_diff):
    pytest.importorskip("scipy")
    d, e = sj.random_field(shape, seed=sum(shape))
    assert _same(sj.labels_by_propagation(d, e, max_diff), sj.labels_by_graph(d, e, max_diff))


@pytest.mark.parametrize("name,make,max_diff", STRUCTURES, ids=[s[0] for s in STRUCTURES])
def test_judge_forms_agree_on_the_structures(name, make, max_diff):
    pytest.importorskip("scipy")
    d = make()
    d3 = d if d.ndim == 3 else d[None]
    assert _same(sj.labels_by_propagation(d3, None, max_diff), sj.labels_by_graph(d3, None, max_diff))


def test_the_structures_are_what_their_names_say():
    lab, size = sj.labels_by_propagation(sj.serpentine(), None, 1.0)
    assert size[0, 0, 0] == 1820 and (lab[0] == 0).sum() == 1820
    lab, size = sj.labels_by_propagation(sj.checkerboard(), None, 0.0)
    assert (size == 1).all() and np.array_equal(lab[0].ravel(), np.arange(35 * 67))
    lab, size = sj.labels_by_propagation(sj.constant_pair(), None, 1.0)
    assert (lab == 0).all() and (size == 9100).all()
    lab, size = sj.labels_by_propagation(sj.spiral(), None, 1.0)
    assert sj.component_sizes(lab, size).size == 2
    lab, size = sj.labels_by_propagation(sj.comb(), None, 1.0)
    assert size[0, 0, 0] == 40 * 67 + 66 and (sj.component_sizes(lab, size) == 39).sum() == 66


def test_random_recipe_has_components_on_both_sides_of_max_size():
    d, e = sj.random_field((1, 67, 131), seed=0)
    lab, size = sj.labels_by_propagation(d, e, 1.0)
    n = sj.component_sizes(lab, size)
    print(f"{n.size} components, {(n <= 20).sum()} of at most 20 px, {(n > 20).sum()} larger")
    assert (n <= 20).sum() >= 50 and (n > 20).sum() >= 50


# ------------------------------------------------------------------ hand-checked 5 x 5 cases
def _five(rows):
    return np.array(rows, np.float32)


def test_rule_wall_splits_and_keeps_its_flag():
    d = np.zeros((5, 5), np.float32)
    e = np.zeros((5, 5), np.uint8)
    e[:, 2] = 2            # a wall down the middle column, flag 2
    e[4, 2] = 0            # ... with a door in the last row
    j = sj.judge(d, e, 0.0, 3)
    assert (j["labels"][:4, 2] == -1).all() and (j["size"][:4, 2] == 0).all()
    assert (j["state"][:4, 2] == 2).all()                     # the flag comes back, not 3
    rest = np.ones((5, 5), bool)
    rest[:4, 2] = False
    assert (j["labels"][rest] == 0).all() and (j["size"][rest] == 21).all() and (j["state"][rest] == 0).all()
    e[4, 2] = 1            # door shut: two components of 10, labels 0 and 3
    j = sj.judge(d, e, 0.0, 3)
    assert (j["labels"][:, :2] == 0).all() and (j["labels"][:, 3:] == 3).all()
    assert (j["size"][:, :2] == 10).all() and (j["size"][:, 3:] == 10).all() and j["state"][4, 2] == 1


def test_rule_non_finite_is_a_wall_and_is_removed():
    d = np.zeros((5, 5), np.float32)
    d[2, :] = [np.nan, np.inf, -np.inf, np.nan, np.nan]
    j = sj.judge(d, None, 1.0, 0, fill=-1.0)
    assert (j["labels"][2] == -1).all() and (j["size"][2] == 0).all()
    assert (j["state"][2] == 3).all() and (j["filtered"][2] == -1.0).all()   # no evidence, even at max_size 0
    assert (j["labels"][:2] == 0).all() and (j["labels"][3:] == 15).all() and (j["size"][[0, 1, 3, 4]] == 10).all()
    assert (j["state"][[0, 1, 3, 4]] == 0).all() and (j["filtered"][[0, 1, 3, 4]] == 0).all()
    e = np.zeros((5, 5), np.uint8)
    e[2, 0] = 1            # a NaN under a flag keeps the flag
    assert sj.judge(d, e, 1.0, 0)["state"][2, 0] == 1


def test_rule_max_diff_boundary_is_inclusive_and_pairwise():
    # steps of exactly 0.5 drift from 0 to 2 along a row: one component at max_diff 0.5
    d = np.tile(np.array([0, 0.5, 1.0, 1.5, 2.0], np.float32), (5, 1))
    assert (sj.judge(d, None, 0.5, 0)["size"] == 25).all()
    assert (sj.judge(d, None, np.nextafter(np.float32(0.5), np.float32(0)), 0)["size"] == 5).all()
    # float32: 1 + 2^-23 differs from 1 by exactly 2^-23
    d = np.ones((5, 5), np.float32)
    d[:, 3:] = np.nextafter(np.float32(1), np.float32(2))
    assert (sj.judge(d, None, 2.0 ** -23, 0)["size"] == 25).all()
    j = sj.judge(d, None, 2.0 ** -24, 0)
    assert (j["size"][:, :3] == 15).all() and (j["size"][:, 3:] == 10).all()
    # -0.0 and 0.0 are connected at max_diff 0
    d = np.zeros((5, 5), np.float32)
    d[::2] = -0.0
    assert (sj.judge(d, None, 0.0, 0)["size"] == 25).all()
    # an overflowing difference is not connected
    d = np.full((5, 5), 3e38, np.float32)
    d[:, 2:] = -3e38
    assert (sj.judge(d, None, 3.4e38, 0)["size"][:, :2] == 10).all()


def test_rule_max_size_boundary():
    d = np.zeros((5, 5), np.float32)
    d[0, :4] = 9.0         # a blob of 4
    for max_size, removed in ((3, False), (4, True), (5, True)):
        j = sj.judge(d, None, 1.0, max_size, fill=np.nan)
        assert (j["size"][0, :4] == 4).all() and (j["size"][1:] == 21).all()
        assert (j["state"][0, :4] == (3 if removed else 0)).all() and (j["state"][1:] == 0).all()
        assert np.isnan(j["filtered"][0, :4]).all() == removed and (j["filtered"][1:] == 0).all()
    assert (sj.judge(d, None, 1.0, 0)["state"] == 0).all()       # max_size 0 removes nothing
    assert (sj.judge(d, None, 1.0, 25)["state"] == 3).all()      # max_size >= H * W removes everything


def test_rule_images_of_a_batch_never_connect():
    d = np.zeros((2, 5, 5), np.float32)
    j = sj.judge(d, None, 0.0, 25)
    assert (j["labels"] == 0).all() and (j["size"] == 25).all() and (j["state"] == 3).all()
    assert (sj.judge(d, None, 0.0, 24)["state"] == 0).all()


# ------------------------------------------------------------------ the C entries
def test_header_declares_and_library_exports_the_entries():
    with open(os.path.join(REPO, "include", "leastereo_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW:
        assert f"{name}(" in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define LEA_LR_SPECKLE 3" in header
    res, args = _lib.SIGNATURES["lea_disparity_speckle_f32"]
    assert len(args) == 14 and args[5] is ctypes.c_float and args[6] is ctypes.c_int and args[7] is ctypes.c_float
    assert _lib.SIGNATURES["lea_disparity_speckle_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.ABI_VERSION == 14 and lib.lea_abi_version() == 14  # additive: the number stays


def test_workspace_bytes():
    lib = _lib.load()
    assert lib.lea_disparity_speckle_workspace_bytes(2, 6, 7) == 8 * 84
    assert lib.lea_disparity_speckle_workspace_bytes(1, 2048, 2048) == 8 << 22
    for bad in ((0, 6, 7), (2, -1, 7), (2, 6, 0)):
        assert lib.lea_disparity_speckle_workspace_bytes(*bad) == 0


# B = 2, H = 6, W = 7: a map is 84 elements (336 bytes as f32 / int32, 84 as bytes), the
# workspace 672 bytes.  Fake device addresses, far apart.
D, EX, WS, LAB, SIZ, ST, FIL = (0x10000 * k for k in range(1, 8))
ARGS = dict(disp=P(D), exclude=P(EX), B=2, H=6, W=7, max_diff=1.0, max_size=20, fill=0.0, ws=P(WS), labels=P(LAB),
            size=P(SIZ), state=P(ST), filtered=P(FIL))


def call(**kw):
    a = dict(ARGS, **kw)
    lib = _lib.load()
    rc = lib.lea_disparity_speckle_f32(a["disp"], a["exclude"], a["B"], a["H"], a["W"], a["max_diff"], a["max_size"],
                                       a["fill"], a["ws"], a["labels"], a["size"], a["state"], a["filtered"], None)
    return rc, lib.lea_last_error()


BAD = [(dict(disp=None), b"disp"), (dict(ws=None), b"workspace"),
       (dict(labels=None, size=None, state=None, filtered=None), b"every output is null"),
       (dict(B=0), b"B="), (dict(H=0), b"H="), (dict(W=-7), b"W="), (dict(B=65536), b"B="),
       (dict(B=1, H=1 << 16, W=1 << 15), b"2^31"), (dict(B=1, H=1 << 20, W=1 << 20), b"2^31"),
       (dict(max_diff=-1.0), b"max_diff"), (dict(max_diff=math.nan), b"max_diff"), (dict(max_diff=math.inf), b"max_diff"),
       (dict(max_size=-1), b"max_size"), (dict(ws=P(WS + 2)), b"aligned"),
       (dict(filtered=P(D)), b"filtered overlaps disp"), (dict(labels=P(D + 332)), b"labels overlaps disp"),
       (dict(state=P(EX + 83)), b"state overlaps exclude"), (dict(exclude=P(ST + 83)), b"state overlaps exclude"),
       (dict(size=P(WS + 668)), b"size overlaps the workspace"), (dict(size=P(LAB)), b"size overlaps labels"),
       (dict(state=P(SIZ + 335)), b"state overlaps size"), (dict(filtered=P(ST + 83)), b"filtered overlaps state"),
       (dict(filtered=P(LAB + 332)), b"filtered overlaps labels"),
       (dict(ws=P(D)), b"workspace overlaps disp"), (dict(ws=P(EX - 668)), b"workspace overlaps exclude")]


@pytest.mark.parametrize("kw,word", BAD, ids=lambda v: ",".join(v) if isinstance(v, dict) else "")
def test_refused_arguments(kw, word):
    rc, err = call(**kw)
    assert rc == INVALID, (rc, err)
    assert b"lea_disparity_speckle_f32" in err and word in err, err


def test_optional_arguments_are_not_refused_for_being_null():
    """exclude and any three of the outputs may be NULL: the next check in line is the one that fires."""
    for keep in ("labels", "size", "state", "filtered"):
        kw = {k: None for k in ("labels", "size", "state", "filtered") if k != keep}
        rc, err = call(exclude=None, max_size=-3, fill=math.nan, **kw)
        assert rc == INVALID and b"max_size" in err
    # outputs that just clear their neighbours are no overlap: the shape check fires instead
    rc, err = call(labels=P(D + 336), size=P(D + 672), W=0)
    assert rc == INVALID and b"W=" in err


# ------------------------------------------------------------------ the Python layers
def test_wrapper_refuses_cpu_tensors_and_has_its_constants():
    with pytest.raises(_lib.HipKernelError):  # no CPU path
        kernels.speckle_filter(torch.zeros(1, 6, 7))
    with pytest.raises(ValueError):
        kernels.speckle_filter(torch.zeros(6))
    with pytest.raises(ValueError):
        kernels.speckle_filter(np.zeros((6, 7), np.float32))
    assert kernels.DisparitySpeckle._fields == ("disp", "state", "size", "labels", "filtered")
    assert (kernels.SPECKLE_MAX_SIZE, kernels.SPECKLE_MAX_DIFF, kernels.LR_SPECKLE) == (200, 1.0, 3)
    assert (kernels.LR_CONSISTENT, kernels.LR_INCONSISTENT, kernels.LR_OUT_OF_VIEW) == (0, 1, 2)
    assert sj.LR_SPECKLE == kernels.LR_SPECKLE


def test_predict_flags():
    from leastereo_amd import predict
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt"]
    old = vars(obtain_predict_args(base))
    assert (old["speckle"], old["speckle_diff"]) == (0, 1.0)
    assert predict.speckle_options(obtain_predict_args(base)) is None             # off: no call anywhere
    assert predict.speckle_options(obtain_predict_args(base + ["--speckle_diff=2"])) is None
    new = obtain_predict_args(base + ["--speckle", "150", "--speckle_diff=1.5"])
    assert predict.speckle_options(new) == dict(max_size=150, max_diff=1.5)
    assert predict.speckle_options(obtain_predict_args(base + ["--speckle=50"])) == dict(max_size=50, max_diff=1.0)
    new = vars(new)
    for k in ("speckle", "speckle_diff"):
        old.pop(k), new.pop(k)
    assert old == new              # nothing else moves
    for bad in (["--speckle=-1"], ["--speckle=50", "--speckle_diff=-0.5"], ["--speckle=50", "--speckle_diff=nan"],
                ["--speckle=50", "--speckle_diff=inf"], ["--speckle=0", "--speckle_diff=-1"]):
        with pytest.raises(ValueError):
            predict.speckle_options(obtain_predict_args(base + bad))
    with pytest.raises(NotImplementedError):
        predict.speckle_options(obtain_predict_args(base + ["--speckle=50", "--satellite=1"]))
    with pytest.raises(SystemExit):
        obtain_predict_args(base + ["--speckle=1.5"])


def test_main_refuses_bad_speckle_flags_before_it_needs_a_device():
    from leastereo_amd import predict
    base = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt", "--sceneflow=1"]
    with pytest.raises(ValueError, match="--speckle_diff"):
        predict.main(base + ["--speckle=50", "--speckle_diff=-1"])
    with pytest.raises(ValueError, match="--speckle"):
        predict.main(base + ["--speckle=-4"])


def test_refine_pair_passes_the_speckle_options_on_only_when_asked(monkeypatch):
    from leastereo_amd import predict, scene
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=6", "--crop_width=8", "--data_path=d/", "--test_list=l.txt", "--refine=1"]
    u8 = np.zeros((6, 8, 3), dtype=np.uint8)
    monkeypatch.setattr(predict, "load_images", lambda a, b: (u8, u8))
    monkeypatch.setattr(predict, "load_transform",
                        lambda l, r, ch, cw, device="cuda": (torch.zeros(1, 3, ch, cw), torch.ones(1, 3, ch, cw), 6, 8))
    calls = []
    maps = {k: torch.zeros(1, 6, 8) for k in kernels.DisparityRefined._fields}

    class Model:
        maxdisp = 12

        def forward_refined(self, x, y, **kw):
            calls.append(("forward_refined", kw.get("speckle", "absent")))
            return kernels.DisparityRefined(**maps)

    result = scene.SceneResult(disp=torch.zeros(6, 8), disp_right=torch.zeros(6, 8),
                               state=torch.zeros(6, 8, dtype=torch.uint8), disp_filled=torch.zeros(6, 8))

    def runner(l, r):
        return result
    runner.model = Model()

    def fake_refine_scene(res, left, lam, sigma, iterations, return_support=False, **kw):
        calls.append(("refine_scene", kw.get("speckle", "absent")))
        return torch.zeros(6, 8), torch.zeros(6, 8)
    monkeypatch.setattr(scene, "refine_scene", fake_refine_scene)
    predict.refine_pair(Model(), None, "l", "r", obtain_predict_args(base))
    predict.refine_pair(Model(), runner, "l", "r", obtain_predict_args(base + ["--scene=1"]))
    assert calls == [("forward_refined", "absent"), ("refine_scene", "absent")]
    calls.clear()
    on = ["--speckle=60", "--speckle_diff=2"]
    predict.refine_pair(Model(), None, "l", "r", obtain_predict_args(base + on))
    predict.refine_pair(Model(), runner, "l", "r", obtain_predict_args(base + on + ["--scene=1"]))
    want = dict(max_size=60, max_diff=2.0)
    assert calls == [("forward_refined", want), ("refine_scene", want)]


def _counting(monkeypatch):
    """kernels.speckle_filter and kernels.fgs_refine replaced by recorders that return maps of
    the right shapes on whatever device the input is on."""
    calls = []

    def fake_speckle(disp, exclude=None, max_size=kernels.SPECKLE_MAX_SIZE, max_diff=kernels.SPECKLE_MAX_DIFF,
                     fill=0.0, want_labels=False, want_size=True, want_filtered=True):
        calls.append(("speckle", exclude is not None, max_size, max_diff))
        return kernels.DisparitySpeckle(disp, torch.full(disp.shape, 3, dtype=torch.uint8), None, None, None)

    def fake_refine(guide, disp, conf=None, exclude=None, lam=0, sigma=0, iterations=0, return_support=False):
        calls.append(("refine", None if exclude is None else int(exclude.max())))
        return (disp.clone(), disp.clone()) if return_support else disp.clone()
    monkeypatch.setattr(kernels, "speckle_filter", fake_speckle)
    monkeypatch.setattr(kernels, "fgs_refine", fake_refine)
    return calls


def test_refine_scene_makes_no_speckle_call_unless_asked(monkeypatch):
    from leastereo_amd import scene
    calls = _counting(monkeypatch)
    monkeypatch.setattr(kernels, "standardize_tiles_u8", lambda l, r, o, h, w: (torch.zeros(1, 3, h, w),) * 2)
    res = scene.SceneResult(disp=torch.zeros(6, 8), state=torch.zeros(6, 8, dtype=torch.uint8))
    left = torch.zeros(6, 8, 3, dtype=torch.uint8)
    scene.refine_scene(res, left)
    scene.refine_scene(res, left, speckle=None)
    assert calls == [("refine", 0), ("refine", 0)]
    calls.clear()
    scene.refine_scene(res, left, speckle={})
    scene.refine_scene(res, left, speckle=dict(max_size=9, max_diff=0.5))
    assert calls == [("speckle", True, 200, 1.0), ("refine", 3), ("speckle", True, 9, 0.5), ("refine", 3)]
    with pytest.raises(ValueError):
        scene.refine_scene(res, left, speckle=dict(size=9))
    with pytest.raises(ValueError):
        scene.refine_scene(res, left, speckle=9)
    calls.clear()
    out = scene.speckle_scene(scene.SceneResult(disp=torch.zeros(6, 8)), max_size=7)
    assert calls == [("speckle", False, 7, 1.0)] and out.state.shape == (6, 8)


def test_forward_refined_makes_no_speckle_call_unless_asked(monkeypatch):
    from leastereo_amd.model import LEAStereo
    calls = _counting(monkeypatch)
    monkeypatch.setattr(kernels, "lr_check", lambda dl, dr, thr, want_state=True, want_filled=True:
                        kernels.DisparityLR(dl, dr, torch.zeros(dl.shape, dtype=torch.uint8), None))

    class Exec:
        def run_features(self, fx, fy, maxdisp):
            return torch.zeros(1)

    class Disp:
        def stats(self, cost, radius, fast_exp=False):
            z = torch.zeros(1, 6, 8)
            return kernels.DisparityStats(z, z, z, z)

        def right(self, cost, fast_exp=False):
            return torch.zeros(1, 6, 8)

    class Fake:
        training, precision, maxdisp, disp = False, "f32", 12, Disp()
        check_shape = staticmethod(lambda h, w: None)
        feature = staticmethod(lambda *a: torch.zeros(2, 1))

        class matching:
            executor = staticmethod(lambda: Exec())

    class OnDevice(torch.Tensor):  # a CPU tensor that says it is on the device: nothing here launches
        is_cuda = True

    x = torch.zeros(1, 3, 6, 8).as_subclass(OnDevice)
    with torch.no_grad():
        out = LEAStereo.forward_refined(Fake(), x, x)
        assert calls == [("refine", 0)] and int(out.state.max()) == 0
        calls.clear()
        LEAStereo.forward_refined(Fake(), x, x, speckle=None)
        assert calls == [("refine", 0)]
        calls.clear()
        out = LEAStereo.forward_refined(Fake(), x, x, speckle={})
        assert calls == [("speckle", True, 200, 1.0), ("refine", 3)] and int(out.state.min()) == 3
        calls.clear()
        LEAStereo.forward_refined(Fake(), x, x, speckle=dict(max_size=30))
        assert calls == [("speckle", True, 30, 1.0), ("refine", 3)]
        for bad in (dict(size=3), 5, [("max_size", 3)]):
            with pytest.raises(ValueError):
                LEAStereo.forward_refined(Fake(), x, x, speckle=bad)
    assert kernels.DisparityRefined._fields == ("disp", "disp_refined", "support", "peak", "disp_right", "state")


def test_save_speckle_writes_the_two_files(tmp_path):
    from leastereo_amd import predict
    from PIL import Image
    removed = np.zeros((6, 8), bool)
    removed[2, 3:5] = True
    filt = np.linspace(0, 90, 48, dtype=np.float32).reshape(6, 8)
    predict.save_speckle(str(tmp_path / "0"), removed, filt)
    assert np.array_equal(np.load(tmp_path / "0_despeckled.npy"), filt)
    png = np.asarray(Image.open(tmp_path / "0_speckle.png"))
    assert png.shape == (6, 8) and np.array_equal(png == 255, removed) and set(np.unique(png)) == {0, 255}


def test_asan_driver_is_wired_into_make_asan():
    """`make asan` links the driver with every unit and runs it: asked of make itself (a dry run
    of everything), since the drivers are one list and a pattern rule pair in the Makefile."""
    assert os.path.isfile(os.path.join(REPO, "tests", "asan", "speckle_asan.cpp"))
    plan = subprocess.run(["make", "-n", "-B", "asan"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert plan.returncode == 0, plan.stderr[-2000:]
    link = [l for l in plan.stdout.splitlines() if " -o build/asan/speckle_asan " in l]
    assert len(link) == 1 and "build/asan/speckle_asan_main.o" in link[0] and "build/asan/speckle.o" in link[0]
    assert "ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/speckle_asan" in plan.stdout.splitlines()
