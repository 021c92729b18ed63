"""The training batch transform off the GPU: the two entries are declared, exported and bound;
``data.sample_train_params`` draws what the reference's train_transform drew (the recorded
draws of tests/golden/train_transform.npz, tools/gen_golden_transform.py); the numpy judge
(tests/transform_judge.py) reproduces the reference's outputs bit for bit; the refusals; the
shift reset rule; ``center_params`` against test_transform's geometry; and the argument
checks of the entry through ctypes (nothing launches on a refused call)."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, data, kernels
from tests import transform_judge as J
from tests.golden_util import golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
NEW = ("lea_train_transform_workspace_bytes", "lea_train_transform_u8")


def fixture_cases():
    g = golden("train_transform")
    return [tuple(int(v) for v in row) for row in g["cases"]]


N_CASES = 12


class Recorder:
    """A ``random``-like object: the module's generator, every draw recorded."""

    def __init__(self):
        self.draws = []

    def randint(self, a, b):
        v = random.randint(a, b)
        self.draws.append((a, b, v))
        return v


class Scripted:
    """Hands out prepared values, checking the bounds asked for."""

    def __init__(self, script):
        self.script = list(script)

    def randint(self, a, b):
        lo, hi, v = self.script.pop(0)
        assert (a, b) == (lo, hi), ((a, b), (lo, hi))
        return v


def test_header_declares_and_library_exports_the_entries():
    with open(os.path.join(REPO, "include", "leastereo_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW:
        assert f"{name}(" in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["lea_train_transform_u8"][1]) == 18
    assert _lib.SIGNATURES["lea_train_transform_u8"][1][14] is ctypes.c_float
    assert _lib.ABI_VERSION == 14 and lib.lea_abi_version() == 14  # additive: the number stays
    assert lib.lea_train_transform_workspace_bytes(3) == lib.lea_standardize_workspace_bytes(3) == 3 * 96
    assert lib.lea_train_transform_workspace_bytes(0) == 0
    for name in ("sample_train_params", "center_params", "DeviceTrainTransform", "TrainBatch"):
        assert hasattr(data, name), name
    assert data.TrainBatch._fields == ("left", "right", "target", "n_valid", "params")
    assert callable(kernels.train_transform_u8)


def test_the_fixture_carries_the_cases_the_issue_lists():
    want = ([(10, 14, 6, 8) + f for f in ((1, 0, 0), (0, 1, 0), (0, 0, 0), (1, 0, 3))] +
            [(5, 7, 6, 8) + f for f in ((1, 0, 0), (0, 1, 0), (1, 0, 2))] +
            [(10, 7, 6, 8) + f for f in ((1, 0, 0), (1, 0, 2))] +
            [(6, 8, 6, 8, 1, 0, 0), (6, 8, 6, 8, 1, 0, 2), (6, 14, 6, 8, 1, 0, 0)])
    assert [c[:7] for c in fixture_cases()] == want and len(want) == N_CASES
    g = golden("train_transform")
    assert len(g["4/draws"]) == 0 and len(g["9/draws"]) == 0           # fits, shift 0: no draw at all
    assert g["5/draws"].tolist() == [[0, 1, 1]]                       # fits, use_left=False: the lone coin
    assert g["1/draws"][-1].tolist() == [0, 1, 0]                     # ... and the other coin


@pytest.mark.parametrize("i", range(N_CASES))
def test_sample_train_params_consumes_the_recorded_draws(i):
    g = golden("train_transform")
    h, w, ch, cw, ul, lr, shift, seed = fixture_cases()[i]
    rec = Recorder()
    random.seed(seed)
    params = data.sample_train_params(h, w, ch, cw, bool(ul), bool(lr), shift, rng=rec)
    assert rec.draws == [tuple(r) for r in g[f"{i}/draws"].tolist()]
    # the default rng is the random module itself: same row under the same seed
    random.seed(seed)
    assert data.sample_train_params(h, w, ch, cw, bool(ul), bool(lr), shift) == params
    assert len(params) == 5 and all(isinstance(v, int) for v in params)


@pytest.mark.parametrize("i", range(N_CASES))
def test_the_judge_reproduces_the_reference_bitwise(i):
    """Both forms of the judge: the literal canvas driven by the recorded draws, and the
    params row of ``sample_train_params`` applied as a window with pad."""
    g = golden("train_transform")
    h, w, ch, cw, ul, lr, shift, seed = fixture_cases()[i]
    t = J.standardize(g[f"{i}/left_u8"], g[f"{i}/right_u8"], g[f"{i}/disp_left"], g[f"{i}/disp_right"])
    want = [g[f"{i}/out_left"], g[f"{i}/out_right"], g[f"{i}/out_target"]]
    script = Scripted(tuple(r) for r in g[f"{i}/draws"].tolist())
    *lit, lit_params = J.train_transform(t, ch, cw, bool(ul), bool(lr), shift, rng=script)
    assert script.script == []
    random.seed(seed)
    params = data.sample_train_params(h, w, ch, cw, bool(ul), bool(lr), shift)
    assert tuple(lit_params) == params
    win = J.apply_params(t, params, ch, cw)
    for got in (lit, win):
        for a, b in zip(got, want):
            assert a.dtype == np.float32 and a.shape == b.shape
            assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_the_fixture_exercises_swap_shift_and_reset():
    g = golden("train_transform")
    rows = []
    for i, (h, w, ch, cw, ul, lr, shift, seed) in enumerate(fixture_cases()):
        random.seed(seed)
        rows.append(data.sample_train_params(h, w, ch, cw, bool(ul), bool(lr), shift))
    assert [r[4] for r in rows] == [0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert rows[3][3] < 0 and rows[10][3] > 0                      # shifts of both signs survive
    assert g["8/draws"][1, 2] != 0 and rows[8][3] == 0               # the reset rule zeroed this one
    assert rows[6][0] < 0 or rows[6][1] < 0                          # a window over the pad


def test_refuses_what_the_reference_cannot_crop():
    with pytest.raises(ValueError, match="train_transform"):
        data.sample_train_params(5, 14, 6, 8)
    with pytest.raises(ValueError, match="train_transform"):
        data.sample_train_params(5, 14, 6, 8, shift=2)
    with pytest.raises(ValueError, match="train_transform"):
        data.sample_train_params(10, 14, 6, 8, shift=-1)
    with pytest.raises(ValueError):
        J.train_transform(np.zeros((8, 5, 14), np.float32), 6, 8, rng=random)
    # h == ch, w > cw is a plain crop: both draws, the second over one value
    assert data.sample_train_params(6, 14, 6, 8, rng=Scripted([(0, 6, 5), (0, 0, 0)])) == (0, 5, 5, 0, 0)
    assert data.sample_train_params(6, 14, 6, 8, shift=2, rng=Scripted([(0, 6, 6), (-2, 2, -2), (0, 0, 0)])) \
        == (0, 4, 6, -2, 0)


def test_shift_reset_rule():
    """shift_x is kept only while the shifted window stays on the canvas (common.py:63-64)."""
    # 10x14 -> 6x8, shift 3: canvas = image, start_x in [0, 6]
    keep = data.sample_train_params(10, 14, 6, 8, shift=3, rng=Scripted([(0, 6, 3), (-3, 3, 3), (0, 4, 2)]))
    assert keep == (2, 6, 3, 3, 0)
    right_edge = data.sample_train_params(10, 14, 6, 8, shift=3, rng=Scripted([(0, 6, 4), (-3, 3, 3), (0, 4, 2)]))
    assert right_edge == (2, 4, 4, 0, 0)                                     # 4 + 3 + 8 > 14
    at_edge = data.sample_train_params(10, 14, 6, 8, shift=3, rng=Scripted([(0, 6, 3), (-3, 3, 3), (0, 4, 0)]))
    assert at_edge[3] == 3                                                   # 3 + 3 + 8 == 14 stays
    left_edge = data.sample_train_params(10, 14, 6, 8, shift=3, rng=Scripted([(0, 6, 2), (-3, 3, -3), (0, 4, 1)]))
    assert left_edge == (1, 2, 2, 0, 0)                                      # 2 - 3 < 0
    # padded canvas (5x7 -> 6x8, shift 2: 8x10, image at (3, 3)): offsets are relative to the image
    padded = data.sample_train_params(5, 7, 6, 8, shift=2, rng=Scripted([(0, 2, 1), (-2, 2, -1), (0, 2, 2)]))
    assert padded == (2 - 3, 0 - 3, 1 - 3, -1, 0)
    # the use_left / left_right coin is not drawn on the shift path
    s = Scripted([(0, 2, 0), (-2, 2, 0), (0, 2, 0)])
    assert data.sample_train_params(5, 7, 6, 8, use_left=False, left_right=True, shift=2, rng=s)[4] == 0
    assert s.script == []


def test_swap_rule():
    for coin, lr, swap in ((0, True, 0), (1, True, 1), (0, False, 1), (1, False, 1)):
        row = data.sample_train_params(5, 7, 6, 8, use_left=False, left_right=lr, rng=Scripted([(0, 1, coin)]))
        assert row == (-1, -1, -1, 0, swap)
    assert data.sample_train_params(5, 7, 6, 8, use_left=True, left_right=True, rng=Scripted([])) == (-1, -1, -1, 0, 0)


@pytest.mark.parametrize("h,w,ch,cw", [(5, 7, 6, 8), (6, 8, 6, 8), (10, 14, 6, 8), (11, 15, 6, 8), (6, 14, 6, 8),
                                       (10, 8, 6, 8)])
def test_center_params_is_the_test_transform_geometry(h, w, ch, cw):
    rng = np.random.default_rng(h * w)
    t = rng.standard_normal((8, h, w)).astype(np.float32)
    row = data.center_params(h, w, ch, cw)
    assert row[3] == 0 and row[4] == 0 and row[1] == row[2]
    for a, b in zip(J.apply_params(t, row, ch, cw), J.test_transform(t, ch, cw)):
        assert np.array_equal(a, b)


def test_center_params_raises_where_standardize_crop_raises():
    for h, w in ((5, 14), (10, 7)):
        with pytest.raises(ValueError, match="test_transform"):
            data.center_params(h, w, 6, 8)
        with pytest.raises(ValueError):
            J.test_transform(np.zeros((8, h, w), np.float32), 6, 8)


def test_judge_window_takes_any_offsets():
    t = np.arange(8 * 3 * 4, dtype=np.float32).reshape(8, 3, 4)
    big = 2 ** 31 - 1
    for row in ((big, 0, 0, 0, 0), (0, -big, big, big, 0), (-big, big, -big, -big, 1 | 0x70)):
        left, right, target = J.apply_params(t, row, 2, 5)
        assert not left.any() and not right.any()
        pad = 0.0 if row[4] & 1 else 1000.0
        assert np.array_equal(target, np.full((1, 2, 5), np.float32(pad) - np.float32(row[3])))


# B = 2, H = 6, W = 7, crop 4x8.  Fake device addresses: the checks compare and never dereference.
ARGS = dict(left=P(0x10000), right=P(0x20000), B=2, H=6, W=7, ps=3, dl=P(0x30000), dr=P(0x40000),
            params=P(0x50000), ol=P(0x60000), orr=P(0x70000), ot=P(0x80000), ch=4, cw=8, md=48.0,
            nv=P(0x90000), ws=P(0xA0000))


def call_entry(**kw):
    a = dict(ARGS, **kw)
    lib = _lib.load()
    rc = lib.lea_train_transform_u8(a["left"], a["right"], a["B"], a["H"], a["W"], a["ps"], a["dl"], a["dr"],
                                    a["params"], a["ol"], a["orr"], a["ot"], a["ch"], a["cw"], a["md"], a["nv"],
                                    a["ws"], None)
    return rc, lib.lea_last_error()


@pytest.mark.parametrize("kw", [
    dict(left=None), dict(right=None), dict(dl=None), dict(params=None), dict(ol=None), dict(orr=None),
    dict(ot=None), dict(ws=None), dict(B=0), dict(B=-1), dict(H=0), dict(W=-7), dict(ch=0), dict(cw=-8),
    dict(ps=2), dict(ps=5), dict(H=1 << 16, W=1 << 15), dict(ch=1 << 16, cw=1 << 15), dict(md=float("nan")),
    dict(ot=P(0x80004)), dict(ol=P(0x60008)), dict(params=P(0x50002)), dict(nv=P(0x90001)), dict(ws=P(0xA0004)),
], ids=lambda v: ",".join(v))
def test_entry_refused_arguments(kw):
    rc, err = call_entry(**kw)
    assert rc == 1001, (rc, err)
    assert b"lea_train_transform_u8" in err, err


@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="needs make and hipcc")
def test_transform_argument_checks_under_asan():
    """`make asan` runs the stand-alone drivers (host code, own main); the transform entries'
    (tests/asan/transform_asan.cpp) prints its own OK line."""
    r = subprocess.run(["make", "-s", "-j8", "asan"], cwd=REPO, capture_output=True, text=True, timeout=1200)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "OK transform: 0 failed checks" in r.stdout, tail
    assert "AddressSanitizer" not in r.stderr, tail


def test_wrapper_refuses_cpu_tensors_and_bad_shapes():
    u8 = torch.zeros(1, 6, 7, 3, dtype=torch.uint8)
    d = torch.zeros(1, 6, 7)
    p = torch.zeros(1, 5, dtype=torch.int32)
    with pytest.raises(_lib.HipKernelError):  # no CPU path
        kernels.train_transform_u8(u8, u8, d, None, p, 4, 8, 48.0)
    with pytest.raises(_lib.HipKernelError):
        data.DeviceTrainTransform(4, 8, 48.0, device="cpu")(u8, u8, d)
