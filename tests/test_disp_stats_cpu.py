"""The confidence head off the GPU: lea_disparity_regression_stats' argument checks through
ctypes (nothing launches on a refused call), DisparityStats.confidence, the predict CLI's
--confidence / --conf_radius flags, and the host AddressSanitizer run of the entry's own
stand-alone driver (tests/asan/disp_stats_asan.cpp, built and run by `make asan`)."""
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
ENTRY = b"lea_disparity_regression_stats"

# B = 1, D3 = 4, H3 = W3 = 2, maxdisp 12: the cost spans 64 bytes, every output 144.  Fake
# device addresses, far apart: the checks compare them and never dereference.
COST, DISP, ENT, PEAK, LOC = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))
GOOD = dict(cost=COST, disp=DISP, entropy=ENT, peak=PEAK, local=LOC, B=1, D3=4, H3=2, W3=2, maxdisp=12,
            radius=4, dtype=0)


def call(**kw):
    a = dict(GOOD, **kw)
    lib = _lib.load()
    rc = lib.lea_disparity_regression_stats(a["cost"], a["disp"], a["entropy"], a["peak"], a["local"], a["B"],
                                            a["D3"], a["H3"], a["W3"], a["maxdisp"], a["radius"], a["dtype"], None)
    return rc, lib.lea_last_error()


@pytest.mark.parametrize("kw,want", [
    (dict(cost=None), INVALID),
    (dict(disp=None), INVALID),
    (dict(entropy=None, peak=None, local=None), INVALID),
    (dict(B=0), INVALID), (dict(D3=0), INVALID), (dict(H3=-1), INVALID), (dict(W3=0), INVALID),
    (dict(maxdisp=0), INVALID),
    (dict(radius=0), INVALID), (dict(radius=17), INVALID), (dict(radius=-4), INVALID),
    (dict(dtype=2), UNSUPPORTED), (dict(dtype=-1), UNSUPPORTED),
    (dict(maxdisp=13), UNSUPPORTED), (dict(maxdisp=8), UNSUPPORTED), (dict(D3=5), UNSUPPORTED),
    (dict(entropy=DISP), INVALID),                                   # two outputs, one buffer
    (dict(peak=ctypes.c_void_p(0x30000 + 140)), INVALID),            # peak starts inside entropy
    (dict(entropy=None, local=PEAK), INVALID),                       # aliasing with a hole beside it
    (dict(disp=COST), INVALID),                                      # in place
    (dict(local=ctypes.c_void_p(0x10000 + 60)), INVALID),            # starts in the cost's last element
    (dict(cost=ctypes.c_void_p(0x20000 + 140)), INVALID),            # cost starts inside disp
], ids=lambda v: ",".join(v) if isinstance(v, dict) else str(v))
def test_refused_arguments(kw, want):
    rc, err = call(**kw)
    assert rc == want, (rc, err)
    assert ENTRY in err, err


def test_signature_is_bound():
    res, args = _lib.SIGNATURES["lea_disparity_regression_stats"]
    assert res is ctypes.c_int and len(args) == 13
    assert _lib.ABI_VERSION == 14 and _lib.load().lea_abi_version() == 14


def test_confidence_arithmetic():
    ent = torch.tensor([[0.0, math.log(48.0) / 2, math.log(48.0)]])
    st = kernels.DisparityStats(torch.zeros(1, 3), ent, None, None, maxdisp=48)
    assert torch.allclose(st.confidence, torch.tensor([[1.0, 0.5, 0.0]]), atol=1e-7)
    disp, entropy, peak, local = st  # a four-field tuple
    assert entropy is ent and peak is None and local is None
    assert st._fields == ("disp", "entropy", "peak", "disp_local") and st.maxdisp == 48
    with pytest.raises(ValueError):
        kernels.DisparityStats(torch.zeros(1, 3), None, ent, None, maxdisp=48).confidence


def test_wrapper_refuses_before_the_library():
    with pytest.raises(_lib.HipKernelError):  # no CPU path
        kernels.disparity_regression_stats(torch.zeros(1, 1, 4, 2, 2), 12)


BASE = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt"]


def test_predict_flags():
    old = vars(obtain_predict_args(BASE))
    assert old["confidence"] == "none" and old["conf_radius"] == 4
    new = vars(obtain_predict_args(BASE + ["--confidence=peak", "--conf_radius=7"]))
    assert new["confidence"] == "peak" and new["conf_radius"] == 7
    assert vars(obtain_predict_args(BASE + ["--confidence", "entropy"]))["confidence"] == "entropy"
    # nothing else moves: every other flag parses to what it did
    for d in (old, new):
        d.pop("confidence"), d.pop("conf_radius")
    assert old == new
    assert old["maxdisp"] == 192 and old["save_path"] == "./result/" and old["precision"] == "f32"
    with pytest.raises(SystemExit):
        obtain_predict_args(BASE + ["--confidence=variance"])


@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="needs make and hipcc")
def test_stats_argument_checks_under_asan():
    """`make asan` runs both stand-alone drivers; the second prints its own OK line."""
    r = subprocess.run(["make", "-s", "-j8", "asan"], cwd=REPO, capture_output=True, text=True, timeout=1200)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "OK: 0 failed checks" in r.stdout, tail
    assert "OK disp_stats: 0 failed checks" in r.stdout, tail
    assert "AddressSanitizer" not in r.stderr, tail
