"""The disparity refinement off the GPU: the judge of tests/refine_judge.py against a dense
solve of the assembled systems, its fixed point, what it is good for on a scene with outliers;
the two new entries are declared, exported and bound, and refuse bad arguments through ctypes
before anything launches; the predict flags and the path --refine takes with and without
--scene (mocked model)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels
from tests import refine_judge as rj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1001
P = ctypes.c_void_p
NEW = ("lea_disparity_refine_workspace_bytes", "lea_disparity_refine_f32")


def test_judge_is_the_dense_solve():
    """refine64's Thomas sweeps against numpy.linalg.solve of I + lambda_t L_h, then
    I + lambda_t L_v, assembled edge by edge: the judge restates the mathematics, not itself."""
    rng = np.random.default_rng(3)
    guide, _ = rj.piecewise_guide(rng, 2, 2, 5, 7)
    disp = rng.uniform(0, 90, size=(2, 5, 7)).astype(np.float32)
    conf = rng.uniform(0.05, 1, size=(2, 5, 7)).astype(np.float32)
    conf[rng.uniform(size=conf.shape) < 0.3] = 0
    exclude = (rng.uniform(size=conf.shape) < 0.1).astype(np.uint8)
    for lam, sigma in ((4.0, 0.5), (128.0, 0.1)):
        got = rj.refine64(guide, disp, conf, exclude, lam, sigma, 2)
        want, den = rj.dense64(guide, disp, conf, exclude, lam, sigma, 2)
        assert got["solved"].all()
        e, ed = np.abs(got["refined"] - want).max(), np.abs(got["den"] - den).max()
        print(f"lambda {lam} sigma {sigma}: judge vs dense solve {e:.3e} (refined), {ed:.3e} (den)")
        assert e <= 1e-12 and ed <= 1e-12


def test_constant_disparity_is_a_fixed_point():
    rng = np.random.default_rng(4)
    guide, _ = rj.piecewise_guide(rng, 2, 3, 9, 33)
    conf = rng.uniform(0.01, 1, size=(2, 9, 33)).astype(np.float32)
    disp = np.full((2, 9, 33), 37.25, dtype=np.float32)
    for T in (1, 3):
        got = rj.refine64(guide, disp, conf, None, 8000.0, 0.05, T)
        e = np.abs(got["refined"] - 37.25).max()
        print(f"T {T}: constant 37.25 moves by {e:.3e}")
        assert got["solved"].all() and e <= 1e-12


def test_outliers_under_zero_confidence_are_filled_from_their_side_of_the_edge():
    """48 x 96, three constant regions whose guide edges are the disparity's; 30 % of the pixels
    replaced by uniform outliers with conf = 0: the mean error falls below 1 % of the input's."""
    rng = np.random.default_rng(5)
    H, W = 48, 96
    labels = np.zeros((1, H, W), dtype=np.int64)
    labels[:, :, 40:] = 1
    labels[:, 20:, 60:] = 2
    truth = np.array([12.0, 40.0, 75.0], dtype=np.float32)[labels]
    guide = np.array([-1.0, 0.5, 1.5], dtype=np.float32)[labels][:, None] + \
        rng.normal(0, 0.01, size=(1, 1, H, W)).astype(np.float32)
    bad = rng.uniform(size=(1, H, W)) < 0.3
    disp = np.where(bad, rng.uniform(0, 90, size=(1, H, W)), truth).astype(np.float32)
    conf = np.where(bad, 0.0, 1.0).astype(np.float32)
    e_in = float(np.abs(disp - truth).mean())
    for lam, sigma in ((8000.0, 0.05), (128.0, 0.1)):
        got = rj.refine64(guide, disp, conf, None, lam, sigma, 3)
        e_out = float(np.abs(got["refined"] - truth).mean())
        print(f"lambda {lam} sigma {sigma}: mean error {e_in:.3f} px -> {e_out:.5f} px")
        assert got["solved"].all() and e_out < 0.01 * e_in


def test_float32_judge_is_close_to_the_float64_one():
    """refine32 only measures float32's own cost; it must not be a different computation."""
    guide, disp, conf = rj.make_case((2, 3, 5, 7), seed=1)
    a, b = rj.refine64(guide, disp, conf, None, 128.0, 0.1, 3), rj.refine32(guide, disp, conf, None, 128.0, 0.1, 3)
    assert b["refined"].dtype == np.float32 and b["den"].dtype == np.float32
    e = np.abs(a["refined"] - b["refined"]).max()
    print(f"E32 = {e:.3e}")
    assert 0 < e < 1e-3


def test_header_declares_and_library_exports_the_entries():
    with open(os.path.join(REPO, "include", "leastereo_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW:
        assert f"{name}(" in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    res, args = _lib.SIGNATURES["lea_disparity_refine_f32"]
    assert len(args) == 16 and args[1] is ctypes.c_int64 and args[9] is ctypes.c_float and args[10] is ctypes.c_float
    assert _lib.SIGNATURES["lea_disparity_refine_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.ABI_VERSION == 14 and lib.lea_abi_version() == 14  # additive: the number stays


def test_workspace_bytes():
    lib = _lib.load()
    assert lib.lea_disparity_refine_workspace_bytes(2, 6, 7) == 7 * 4 * 84
    assert lib.lea_disparity_refine_workspace_bytes(1, 2048, 2048) == 28 << 22
    for bad in ((0, 6, 7), (2, -1, 7), (2, 6, 0)):
        assert lib.lea_disparity_refine_workspace_bytes(*bad) == 0


# B = 2, C = 3, H = 6, W = 7: the guide spans 2 * 126 floats = 1008 bytes, a map 84 floats =
# 336 bytes (exclude: 84 bytes), the workspace 7 * 336 = 2352 bytes.  Fake device addresses,
# far apart: the checks compare them and never dereference.
G, D, CF, EX, WS, OUT, SUP = (0x10000 * k for k in range(1, 8))
ARGS = dict(guide=P(G), gbs=126, disp=P(D), conf=P(CF), exclude=P(EX), B=2, C=3, H=6, W=7, lam=8000.0, sigma=0.05,
            T=3, ws=P(WS), refined=P(OUT), support=P(SUP))


def call(**kw):
    a = dict(ARGS, **kw)
    lib = _lib.load()
    rc = lib.lea_disparity_refine_f32(a["guide"], a["gbs"], a["disp"], a["conf"], a["exclude"], a["B"], a["C"],
                                      a["H"], a["W"], a["lam"], a["sigma"], a["T"], a["ws"], a["refined"],
                                      a["support"], None)
    return rc, lib.lea_last_error()


BAD = [(dict(guide=None), b"guide"), (dict(disp=None), b"disp"), (dict(ws=None), b"workspace"),
       (dict(refined=None), b"refined"), (dict(B=0), b"B="), (dict(H=0), b"H="), (dict(W=-7), b"W="),
       (dict(B=32768), b"grid"), (dict(H=(1 << 21) + 1, W=1, gbs=1 << 23), b"grid"), (dict(H=1 << 20, W=1 << 20, gbs=3 << 40), b"grid"),
       (dict(C=0), b"C="), (dict(C=5, gbs=210), b"C="), (dict(C=-1), b"C="),
       (dict(T=0), b"iterations"), (dict(T=9), b"iterations"), (dict(T=-3), b"iterations"),
       (dict(lam=0.0), b"lambda"), (dict(lam=-1.0), b"lambda"), (dict(lam=math.nan), b"lambda"),
       (dict(lam=math.inf), b"lambda"), (dict(sigma=0.0), b"sigma"), (dict(sigma=-0.05), b"sigma"),
       (dict(sigma=math.nan), b"sigma"), (dict(sigma=math.inf), b"sigma"),
       (dict(gbs=125), b"guide batch stride"), (dict(gbs=0), b"guide batch stride"),
       (dict(ws=P(WS + 2)), b"aligned"),
       (dict(refined=P(D)), b"refined overlaps disp"), (dict(refined=P(G + 1004)), b"refined overlaps guide"),
       (dict(gbs=168, refined=P(G + 4 * (168 + 125))), b"refined overlaps guide"),
       (dict(refined=P(CF + 332)), b"refined overlaps conf"), (dict(refined=P(EX + 83)), b"refined overlaps exclude"),
       (dict(exclude=P(OUT + 335)), b"refined overlaps exclude"),
       (dict(refined=P(WS + 2348)), b"refined overlaps the workspace"),
       (dict(support=P(D + 332)), b"support overlaps disp"), (dict(support=P(G)), b"support overlaps guide"),
       (dict(support=P(WS + 672)), b"support overlaps the workspace"),
       (dict(support=P(OUT + 332)), b"refined overlaps support"), (dict(support=P(OUT)), b"refined overlaps support"),
       (dict(ws=P(CF)), b"workspace overlaps conf"), (dict(ws=P(D - 2348)), b"workspace overlaps disp"),
       (dict(ws=P(G + 1004)), b"workspace overlaps guide")]


@pytest.mark.parametrize("kw,word", BAD, ids=lambda v: ",".join(v) if isinstance(v, dict) else "")
def test_refused_arguments(kw, word):
    rc, err = call(**kw)
    assert rc == INVALID, (rc, err)
    assert b"lea_disparity_refine_f32" in err and word in err, err


def test_optional_arguments_are_not_refused_for_being_null():
    """conf, exclude and support may be NULL: the next check in line is the one that fires."""
    rc, err = call(conf=None, exclude=None, support=None, T=0)
    assert rc == INVALID and b"iterations" in err
    # a refined that just clears its neighbours is no overlap: the shape check fires instead
    rc, err = call(refined=P(D + 336), support=P(D + 672), W=0)
    assert rc == INVALID and b"W=" in err


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    g, d = torch.zeros(1, 3, 6, 7), torch.zeros(1, 6, 7)
    with pytest.raises(_lib.HipKernelError):  # no CPU path
        kernels.fgs_refine(g, d)
    assert kernels.DisparityRefined._fields == ("disp", "disp_refined", "support", "peak", "disp_right", "state")
    assert (kernels.REFINE_LAMBDA, kernels.REFINE_SIGMA, kernels.REFINE_ITERATIONS) == (8000.0, 0.05, 3)


def test_predict_flags():
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt"]
    old = vars(obtain_predict_args(base))
    assert (old["refine"], old["refine_lambda"], old["refine_sigma"], old["refine_iters"]) == (0, 8000.0, 0.05, 3)
    new = vars(obtain_predict_args(base + ["--refine", "1", "--refine_lambda=128", "--refine_sigma", "0.1",
                                           "--refine_iters=2"]))
    assert (new["refine"], new["refine_lambda"], new["refine_sigma"], new["refine_iters"]) == (1, 128.0, 0.1, 2)
    for k in ("refine", "refine_lambda", "refine_sigma", "refine_iters"):
        old.pop(k), new.pop(k)
    assert old == new              # nothing else moves


class _Recorder:
    def __init__(self):
        self.calls = []


def test_refine_takes_the_pair_path_without_scene_and_the_scene_path_with_it(monkeypatch):
    from leastereo_amd import predict, scene
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=6", "--crop_width=8", "--data_path=d/", "--test_list=l.txt", "--refine=1",
            "--refine_lambda=128", "--refine_sigma=0.1", "--refine_iters=2", "--conf_radius=3"]
    u8 = np.zeros((6, 8, 3), dtype=np.uint8)
    monkeypatch.setattr(predict, "load_images", lambda a, b: (u8, u8))
    monkeypatch.setattr(predict, "load_transform",
                        lambda l, r, ch, cw, device="cuda": (torch.zeros(1, 3, ch, cw), torch.ones(1, 3, ch, cw), 6, 8))
    rec = _Recorder()
    maps = {k: torch.full((1, 6, 8), float(i)) for i, k in enumerate(kernels.DisparityRefined._fields)}

    class Model:
        maxdisp = 12

        def forward_refined(self, x, y, **kw):
            rec.calls.append(("forward_refined", kw))
            return kernels.DisparityRefined(**maps)

    # without --scene: one forward_refined on the crop, with the flags' values
    opt = obtain_predict_args(base + ["--lr_check=2"])
    disp, lr, (refined, support) = predict.refine_pair(Model(), None, "l.png", "r.png", opt)
    assert disp is None and lr is None
    assert rec.calls == [("forward_refined", dict(lam=128.0, sigma=0.1, iterations=2, radius=3, lr_threshold=2.0))]
    assert refined.shape == (6, 8) and (refined == 1).all() and (support == 2).all()

    # with --scene: the runner's blended maps go through scene.refine_scene, once; no forward_refined
    rec.calls.clear()
    result = scene.SceneResult(disp=torch.full((6, 8), 5.0), peak=torch.ones(6, 8),
                               disp_right=torch.zeros(6, 8), state=torch.zeros(6, 8, dtype=torch.uint8),
                               disp_filled=torch.zeros(6, 8))

    def runner(l, r):
        rec.calls.append(("runner",))
        return result
    runner.model = Model()

    def fake_refine_scene(res, left, lam, sigma, iterations, return_support=False):
        rec.calls.append(("refine_scene", res is result, left is u8, lam, sigma, iterations, return_support))
        return torch.full((6, 8), 7.0), torch.full((6, 8), 0.5)
    monkeypatch.setattr(scene, "refine_scene", fake_refine_scene)
    opt = obtain_predict_args(base + ["--scene=1"])
    disp, lr, (refined, support) = predict.refine_pair(Model(), runner, "l.png", "r.png", opt)
    assert rec.calls == [("runner",), ("refine_scene", True, True, 128.0, 0.1, 2, True)]
    assert (disp == 5).all() and lr is not None and (refined == 7).all() and (support == 0.5).all()


def test_save_refined_writes_the_three_files(tmp_path):
    from leastereo_amd import predict
    refined = np.linspace(0, 90, 48, dtype=np.float32).reshape(6, 8)
    predict.save_refined(str(tmp_path / "0"), refined, np.linspace(0, 1.2, 48).reshape(6, 8))
    from PIL import Image
    assert np.array_equal(np.load(tmp_path / "0_refined.npy"), refined)
    assert Image.open(tmp_path / "0_refined.png").size == (8, 6)
    assert Image.open(tmp_path / "0_support.png").size == (8, 6)


def test_asan_driver_is_wired_into_make_asan():
    """`make asan` links the driver with every unit and runs it: asked of make itself (a dry run
    of everything), since the drivers are one list and a pattern rule pair in the Makefile."""
    assert os.path.isfile(os.path.join(REPO, "tests", "asan", "refine_asan.cpp"))
    plan = subprocess.run(["make", "-n", "-B", "asan"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert plan.returncode == 0, plan.stderr[-2000:]
    link = [l for l in plan.stdout.splitlines() if " -o build/asan/refine_asan " in l]
    assert len(link) == 1 and "build/asan/refine_asan_main.o" in link[0] and "build/asan/refine.o" in link[0]
    assert "ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/refine_asan" in plan.stdout.splitlines()
