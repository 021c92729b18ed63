"""The left-right check off the GPU: the argument checks of lea_disparity_regression_right and
lea_disparity_lr_check through ctypes (nothing launches on a refused call), DisparityLR, the
predict CLI's --lr_check flag, the wrappers' CPU refusals, and the host AddressSanitizer run
of the entries' own stand-alone driver (tests/asan/lr_asan.cpp, built and run by `make asan`)."""
import ctypes
import math
import os
import shutil
import subprocess

import pytest
import torch

from leastereo_amd import _lib, kernels
from leastereo_amd.config import obtain_predict_args

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1001, 1002
P = ctypes.c_void_p

# right head: B = 1, D3 = 4, H3 = W3 = 2, maxdisp 12: the cost spans 64 bytes, the output 144.
# Fake device addresses, far apart: the checks compare them and never dereference.
RIGHT = dict(cost=P(0x10000), out=P(0x20000), B=1, D3=4, H3=2, W3=2, maxdisp=12, dtype=0)


def call_right(**kw):
    a = dict(RIGHT, **kw)
    lib = _lib.load()
    rc = lib.lea_disparity_regression_right(a["cost"], a["out"], a["B"], a["D3"], a["H3"], a["W3"], a["maxdisp"],
                                            a["dtype"], None)
    return rc, lib.lea_last_error()


@pytest.mark.parametrize("kw,want", [
    (dict(cost=None), INVALID), (dict(out=None), INVALID),
    (dict(B=0), INVALID), (dict(D3=0), INVALID), (dict(D3=-4), INVALID), (dict(H3=-1), INVALID),
    (dict(W3=0), INVALID), (dict(maxdisp=0), INVALID), (dict(maxdisp=-12), INVALID),
    (dict(dtype=2), UNSUPPORTED), (dict(dtype=-1), UNSUPPORTED),
    (dict(maxdisp=13), UNSUPPORTED), (dict(maxdisp=8), UNSUPPORTED), (dict(D3=5), UNSUPPORTED),
    (dict(out=P(0x10000)), INVALID),                 # in place
    (dict(out=P(0x10000 + 60)), INVALID),            # starts in the cost's last element
    (dict(cost=P(0x20000 + 140)), INVALID),          # cost starts in the output's last element
], ids=lambda v: ",".join(v) if isinstance(v, dict) else str(v))
def test_right_refused_arguments(kw, want):
    rc, err = call_right(**kw)
    assert rc == want, (rc, err)
    assert b"lea_disparity_regression_right" in err, err


# check: B = 1, H = W = 6: the float maps span 144 bytes, the states 36
DL, DR, ST, FI = 0x10000, 0x20000, 0x30000, 0x40000
CHECK = dict(dl=P(DL), dr=P(DR), state=P(ST), filled=P(FI), B=1, H=6, W=6, thr=1.0)


def call_check(**kw):
    a = dict(CHECK, **kw)
    lib = _lib.load()
    rc = lib.lea_disparity_lr_check(a["dl"], a["dr"], a["state"], a["filled"], a["B"], a["H"], a["W"], a["thr"], None)
    return rc, lib.lea_last_error()


@pytest.mark.parametrize("kw", [
    dict(dl=None), dict(dr=None), dict(state=None, filled=None),
    dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=-6), dict(W=-6),
    dict(thr=0.0), dict(thr=-1.0), dict(thr=math.nan), dict(thr=math.inf),
    # every (output, input) and (output, output) pair
    dict(state=P(DL)), dict(state=P(DL + 143)), dict(dl=P(ST + 35)),        # state x disp_left
    dict(state=P(DR)), dict(state=P(DR + 143)), dict(dr=P(ST + 35)),        # state x disp_right
    dict(filled=P(DL)), dict(filled=P(DL + 140)), dict(dl=P(FI + 140)),     # filled x disp_left
    dict(filled=P(DR)), dict(filled=P(DR + 140)), dict(dr=P(FI + 140)),     # filled x disp_right
    dict(state=P(FI)), dict(state=P(FI + 143)), dict(filled=P(ST + 32)),    # state x filled
    dict(state=None, filled=P(DR + 4)), dict(filled=None, state=P(DL + 4)),  # with the other output null
], ids=lambda v: ",".join(v))
def test_check_refused_arguments(kw):
    rc, err = call_check(**kw)
    assert rc == INVALID, (rc, err)
    assert b"lea_disparity_lr_check" in err, err


def test_signatures_are_bound():
    res, args = _lib.SIGNATURES["lea_disparity_regression_right"]
    assert res is ctypes.c_int and len(args) == 9
    res, args = _lib.SIGNATURES["lea_disparity_lr_check"]
    assert res is ctypes.c_int and len(args) == 9 and args[7] is ctypes.c_float
    assert _lib.ABI_VERSION == 14 and _lib.load().lea_abi_version() == 14  # additive: the number stays


def test_disparity_lr_fields_and_constants():
    assert kernels.DisparityLR._fields == ("disp", "disp_right", "state", "disp_filled")
    assert (kernels.LR_CONSISTENT, kernels.LR_INCONSISTENT, kernels.LR_OUT_OF_VIEW) == (0, 1, 2)
    a, b = torch.zeros(1, 2, 3), torch.ones(1, 2, 3)
    lr = kernels.DisparityLR(a, b, None, None)
    disp, right, state, filled = lr
    assert disp is a and right is b and state is None and filled is None


def test_wrappers_refuse_cpu_tensors():
    with pytest.raises(_lib.HipKernelError):  # no CPU path
        kernels.disparity_regression_right(torch.zeros(1, 1, 4, 2, 2), 12)
    with pytest.raises(_lib.HipKernelError):
        kernels.lr_check(torch.zeros(1, 6, 6), torch.zeros(1, 6, 6))


BASE = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt"]


def test_predict_flag():
    old = vars(obtain_predict_args(BASE))
    assert old["lr_check"] == 0 and isinstance(old["lr_check"], float)
    new = vars(obtain_predict_args(BASE + ["--lr_check=1.5"]))
    assert new["lr_check"] == 1.5
    assert vars(obtain_predict_args(BASE + ["--lr_check", "2"]))["lr_check"] == 2.0
    # nothing else moves: every other flag parses to what it did
    old.pop("lr_check"), new.pop("lr_check")
    assert old == new
    assert old["maxdisp"] == 192 and old["save_path"] == "./result/" and old["precision"] == "f32"
    assert old["confidence"] == "none" and old["conf_radius"] == 4
    both = vars(obtain_predict_args(BASE + ["--lr_check=1", "--confidence=peak"]))
    assert both["lr_check"] == 1.0 and both["confidence"] == "peak"
    with pytest.raises(SystemExit):
        obtain_predict_args(BASE + ["--lr_check=on"])


@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="needs make and hipcc")
def test_lr_argument_checks_under_asan():
    """`make asan` runs the three stand-alone drivers; each prints its own OK line."""
    r = subprocess.run(["make", "-s", "-j8", "asan"], cwd=REPO, capture_output=True, text=True, timeout=1200)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "OK: 0 failed checks" in r.stdout, tail
    assert "OK disp_stats: 0 failed checks" in r.stdout, tail
    assert "OK lr: 0 failed checks" in r.stdout, tail
    assert "AddressSanitizer" not in r.stderr, tail
