"""Photometric consistency off the GPU: the judge of tests/photo_judge.py against
``F.grid_sample`` and its closed-form gradient against autograd; the three new entries are
declared, exported and bound, and refuse bad arguments through ctypes before anything
launches; the workspace query."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn.functional as F

from leastereo_amd import _lib, kernels, losses
from tests import photo_judge

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1001
P = ctypes.c_void_p
NEW = ("lea_photometric_workspace_bytes", "lea_photometric_f32", "lea_photometric_grad_f32")
SHAPES = [(1, 1, 3, 3), (2, 3, 5, 8), (2, 3, 17, 70), (1, 4, 17, 65)]
IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else s)


@pytest.mark.parametrize("kind", ["grid", "float"])
@pytest.mark.parametrize("shape", SHAPES[1:], **IDS)
def test_the_judges_warp_is_grid_sample(shape, kind):
    """Bilinear, align_corners=True, rows exact, in float64, on the pixels in view."""
    left, right, disp, _ = photo_judge.make_case(shape, kind)
    b, c, h, w = shape
    got, in_view, _ = photo_judge.warp(right, disp, torch.float64)
    xs = (torch.arange(w, dtype=torch.float32).view(1, 1, w) - disp).double()
    gy = torch.linspace(-1, 1, h, dtype=torch.float64).view(1, h, 1).expand(b, h, w)
    grid = torch.stack([2 * xs / (w - 1) - 1, gy], -1)
    want = F.grid_sample(right.double(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    m = in_view.unsqueeze(1).expand_as(got)
    assert 0 < int(in_view.sum()) < in_view.numel()
    err = float((got - want)[m].abs().max())
    print(f"{shape} {kind}: warp vs grid_sample {err:.3e}")
    assert err <= 1e-12            # grid_sample rebuilds xs from the normalised coordinate
    assert bool((got[~m] == 0).all())


@pytest.mark.parametrize("kind", ["grid", "float", "exclude"])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_closed_form_gradient_is_autograd(shape, kind):
    left, right, disp, exclude = photo_judge.make_case(shape, kind)
    for scales in ((1 - photo_judge.ALPHA, photo_judge.ALPHA), (0.0, 1.0), (1.0, 0.0)):
        want = photo_judge.judge(left, right, disp, exclude, scales=scales)["ddisp"]
        got = photo_judge.closed_form_ddisp(left, right, disp, exclude, scales=scales)
        err = float((got - want).abs().max())
        print(f"{shape} {kind} scales {scales}: closed form vs autograd {err:.3e}, max |g| {float(want.abs().max()):.3e}")
        assert err <= 1e-12
        assert float(want.abs().max()) > 0


def test_header_declares_and_library_exports_the_entries():
    with open(os.path.join(REPO, "include", "leastereo_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW:
        assert f"{name}(" in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["lea_photometric_f32"][1]) == 20
    assert len(_lib.SIGNATURES["lea_photometric_grad_f32"][1]) == 19
    assert _lib.ABI_VERSION == 14 and lib.lea_abi_version() == 14  # additive: the number stays


# B = 2, C = 3, H = 6, W = 7: an image spans 2 * 126 floats = 1008 bytes, a map 2 * 42 floats
# = 336 bytes.  Fake device addresses, far apart: the checks compare them and never
# dereference.
L, R, D, EX, SUMS, WS, SC, OUT, WARPED, ERR = (0x10000 * k for k in range(1, 11))
ARGS = dict(left=P(L), lbs=126, right=P(R), rbs=126, disp=P(D), dbs=42, exclude=P(EX), ebs=42, B=2, C=3, H=6, W=7,
            alpha=0.85, c1=1e-4, c2=9e-4, sums=P(SUMS), ws=P(WS), warped=P(WARPED), err=P(ERR), scales=P(SC),
            ddisp=P(OUT), gbs=42)


def call_sums(**kw):
    a = dict(ARGS, **kw)
    lib = _lib.load()
    rc = lib.lea_photometric_f32(a["left"], a["lbs"], a["right"], a["rbs"], a["disp"], a["dbs"], a["exclude"],
                                 a["ebs"], a["B"], a["C"], a["H"], a["W"], a["alpha"], a["c1"], a["c2"], a["sums"],
                                 a["ws"], a["warped"], a["err"], None)
    return rc, lib.lea_last_error()


def call_grad(**kw):
    a = dict(ARGS, **kw)
    lib = _lib.load()
    rc = lib.lea_photometric_grad_f32(a["left"], a["lbs"], a["right"], a["rbs"], a["disp"], a["dbs"], a["exclude"],
                                      a["ebs"], a["B"], a["C"], a["H"], a["W"], a["c1"], a["c2"], a["sums"],
                                      a["scales"], a["ddisp"], a["gbs"], None)
    return rc, lib.lea_last_error()


# (arguments, a word the message must hold)
SHARED_BAD = [(dict(left=None), b"left"), (dict(right=None), b"right"), (dict(disp=None), b"disp"),
              (dict(sums=None), b"sums"), (dict(C=0), b"C="), (dict(C=5), b"C="), (dict(C=-1), b"C="),
              (dict(H=2), b"H="), (dict(W=2), b"W="), (dict(H=0), b"H="), (dict(W=-7), b"W="), (dict(B=0), b"B="),
              (dict(lbs=125), b"left batch stride"), (dict(rbs=0), b"right batch stride"),
              (dict(dbs=41), b"disp batch stride"), (dict(ebs=41), b"exclude batch stride"),
              (dict(c1=0.0), b"c1"), (dict(c1=-1e-4), b"c1"), (dict(c2=0.0), b"c2"), (dict(c2=math.nan), b"c2"),
              (dict(sums=P(SUMS + 4)), b"sums")]
BAD_IDS = dict(ids=lambda v: ",".join(v) if isinstance(v, dict) else "")


@pytest.mark.parametrize("kw,word", SHARED_BAD + [
    (dict(ws=None), b"workspace"), (dict(ws=P(WS + 4)), b"workspace"), (dict(ws=P(SUMS + 8)), b"workspace"),
    (dict(alpha=-0.01), b"alpha"), (dict(alpha=1.5), b"alpha"), (dict(alpha=math.nan), b"alpha"),
    (dict(warped=P(L)), b"warped"), (dict(warped=P(R + 1004)), b"warped"), (dict(err=P(D + 332)), b"err"),
    (dict(err=P(EX + 41)), b"err"), (dict(err=P(WARPED + 1004)), b"err"), (dict(sums=P(L + 8)), b"sums"),
    (dict(ws=P(D)), b"workspace"), (dict(err=P(SUMS + 24)), b"err"), (dict(left=P(ERR + 332)), b"err"),
], **BAD_IDS)
def test_sums_refused_arguments(kw, word):
    rc, err = call_sums(**kw)
    assert rc == INVALID, (rc, err)
    assert b"lea_photometric_f32" in err and word in err, err


@pytest.mark.parametrize("kw,word", SHARED_BAD + [
    (dict(scales=None), b"scales"), (dict(ddisp=None), b"ddisp"), (dict(gbs=41), b"ddisp"),
    (dict(ddisp=P(L)), b"ddisp"), (dict(ddisp=P(R + 1004)), b"ddisp"), (dict(disp=P(OUT + 332)), b"ddisp"),
    (dict(ddisp=P(EX + 83)), b"ddisp"), (dict(ddisp=P(SUMS + 28)), b"ddisp"), (dict(ddisp=P(SC + 4)), b"ddisp"),
], **BAD_IDS)
def test_grad_refused_arguments(kw, word):
    rc, err = call_grad(**kw)
    assert rc == INVALID, (rc, err)
    assert b"lea_photometric_grad_f32" in err and word in err, err


def test_optional_arguments_are_not_refused_for_being_null():
    """exclude, warped and err may be NULL: the next check in line is the one that fires."""
    rc, err = call_sums(exclude=None, ebs=0, warped=None, err=None, alpha=2.0)
    assert rc == INVALID and b"alpha" in err
    rc, err = call_grad(exclude=None, ebs=0, gbs=0)
    assert rc == INVALID and b"ddisp batch stride" in err


def test_workspace_bytes():
    lib = _lib.load()
    for b, h, w in [(1, 3, 3), (2, 17, 70), (1, 17, 65), (4, 288, 576)]:
        n = lib.lea_photometric_workspace_bytes(b, h, w)
        assert n > 0 and n % 8 == 0, (b, h, w, n)
    # one 64 x 16 tile (kPhW, kPhH in csrc/photometric.hip) of four doubles; then 2 x 2 x 2 tiles
    assert lib.lea_photometric_workspace_bytes(1, 3, 3) == 32
    assert lib.lea_photometric_workspace_bytes(2, 17, 65) == 2 * 2 * 2 * 32
    assert lib.lea_photometric_workspace_bytes(0, 17, 65) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    img, d = torch.zeros(1, 3, 6, 7), torch.zeros(1, 6, 7)
    with pytest.raises(_lib.HipKernelError):  # no CPU path
        kernels.photometric_sums(img, img, d)
    with pytest.raises(_lib.HipKernelError):
        kernels.photometric_grad(img, img, d, sums=torch.zeros(4, dtype=torch.float64), scales=torch.ones(2))
    with pytest.raises(_lib.HipKernelError):
        losses.photometric_loss(img, img, d.clone().requires_grad_())
    with pytest.raises(_lib.HipKernelError):
        losses.photometric_loss(img, img, d.unsqueeze(1))


def test_predict_flag():
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt"]
    old, new = vars(obtain_predict_args(base)), vars(obtain_predict_args(base + ["--photo_check"]))
    assert old.pop("photo_check") is False and new.pop("photo_check") is True
    assert old == new              # nothing else moves
    both = vars(obtain_predict_args(base + ["--photo_check", "--lr_check=1"]))
    assert both["photo_check"] and both["lr_check"] == 1.0
