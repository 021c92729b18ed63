"""The edge-aware loss off the GPU: the three new entries are declared, exported and bound;
their argument checks through ctypes (nothing launches on a refused call); the wrappers'
CPU refusals; the two median judges of tests/loss_judge.py agree with each other; and the
host AddressSanitizer run of the entries' stand-alone driver (tests/asan/loss_asan.cpp,
built and run by `make asan`)."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels, losses
from tests import loss_judge

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1001
P = ctypes.c_void_p
NEW = ("lea_median5x5_f32", "lea_edge_loss_workspace_bytes", "lea_edge_loss_f32", "lea_edge_loss_grad_f32")


def test_header_declares_and_library_exports_the_entries():
    with open(os.path.join(REPO, "include", "leastereo_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW:
        assert f"{name}(" in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES["lea_median5x5_f32"][1][1] is ctypes.c_int64
    assert len(_lib.SIGNATURES["lea_median5x5_f32"][1]) == 9
    assert len(_lib.SIGNATURES["lea_edge_loss_f32"][1]) == 13
    assert len(_lib.SIGNATURES["lea_edge_loss_grad_f32"][1]) == 15
    assert _lib.ABI_VERSION == 14 and lib.lea_abi_version() == 14  # additive: the number stays


# B = 2, H = 6, W = 7: a map spans 2 * 42 floats = 336 bytes.  Fake device addresses, far
# apart: the checks compare them and never dereference.
X, Y, TS, SUMS, WS, SC, DP = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
MED = dict(x=P(X), xbs=42, y=P(Y), ybs=42, B=2, H=6, W=7, it=2)


def call_median(**kw):
    a = dict(MED, **kw)
    lib = _lib.load()
    rc = lib.lea_median5x5_f32(a["x"], a["xbs"], a["y"], a["ybs"], a["B"], a["H"], a["W"], a["it"], None)
    return rc, lib.lea_last_error()


@pytest.mark.parametrize("kw", [
    dict(x=None), dict(y=None), dict(it=0), dict(it=3), dict(it=-1),
    dict(xbs=41), dict(ybs=41), dict(xbs=0), dict(ybs=-42),
    dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=-6), dict(W=-7),
    dict(y=P(X)), dict(y=P(X + 332)), dict(x=P(Y + 332)),        # in place, last element either way
], ids=lambda v: ",".join(v))
def test_median_refused_arguments(kw):
    rc, err = call_median(**kw)
    assert rc == INVALID, (rc, err)
    assert b"lea_median5x5_f32" in err, err


LOSS = dict(pred=P(X), pbs=42, target=P(Y), tbs=42, ts=P(TS), sbs=42, B=2, H=6, W=7, md=48.0,
            sums=P(SUMS), ws=P(WS), scales=P(SC), dpred=P(DP), dbs=42)


def call_sums(**kw):
    a = dict(LOSS, **kw)
    lib = _lib.load()
    rc = lib.lea_edge_loss_f32(a["pred"], a["pbs"], a["target"], a["tbs"], a["ts"], a["sbs"], a["B"], a["H"],
                               a["W"], a["md"], a["sums"], a["ws"], None)
    return rc, lib.lea_last_error()


def call_grad(**kw):
    a = dict(LOSS, **kw)
    lib = _lib.load()
    rc = lib.lea_edge_loss_grad_f32(a["pred"], a["pbs"], a["target"], a["tbs"], a["ts"], a["sbs"], a["sums"],
                                    a["scales"], a["dpred"], a["dbs"], a["B"], a["H"], a["W"], a["md"], None)
    return rc, lib.lea_last_error()


SHARED_BAD = [dict(pred=None), dict(target=None), dict(ts=None), dict(sums=None),
              dict(B=0), dict(H=2), dict(W=2), dict(H=0), dict(W=-7), dict(B=-2),
              dict(pbs=41), dict(tbs=41), dict(sbs=0), dict(md=math.nan), dict(sums=P(SUMS + 4))]


@pytest.mark.parametrize("kw", SHARED_BAD + [dict(ws=None), dict(ws=P(WS + 2)), dict(ws=P(SUMS + 8))],
                         ids=lambda v: ",".join(v))
def test_sums_refused_arguments(kw):
    rc, err = call_sums(**kw)
    assert rc == INVALID, (rc, err)
    assert b"lea_edge_loss_f32" in err, err


@pytest.mark.parametrize("kw", SHARED_BAD + [dict(scales=None), dict(dpred=None), dict(dbs=41),
                                             dict(dpred=P(X)), dict(dpred=P(Y + 332)), dict(ts=P(DP + 332)),
                                             dict(dpred=P(SUMS + 28)), dict(dpred=P(SC + 4))],
                         ids=lambda v: ",".join(v))
def test_grad_refused_arguments(kw):
    rc, err = call_grad(**kw)
    assert rc == INVALID, (rc, err)
    assert b"lea_edge_loss_grad_f32" in err, err


def test_workspace_bytes():
    lib = _lib.load()
    # one 64 x 16 tile of four doubles; then 2 x 2 x 2 tiles
    assert lib.lea_edge_loss_workspace_bytes(1, 3, 3) == 32
    assert lib.lea_edge_loss_workspace_bytes(2, 17, 65) == 2 * 2 * 2 * 32
    assert lib.lea_edge_loss_workspace_bytes(0, 17, 65) == 0


def test_wrappers_refuse_cpu_tensors():
    z = torch.zeros(1, 6, 7)
    with pytest.raises(_lib.HipKernelError):  # no CPU path
        kernels.median_blur5(z)
    with pytest.raises(_lib.HipKernelError):
        kernels.edge_loss_sums(z, z, z, 48.0)
    with pytest.raises(_lib.HipKernelError):
        kernels.edge_loss_grad(z, z, z, 48.0, torch.zeros(4, dtype=torch.float64), torch.ones(2))
    with pytest.raises(_lib.HipKernelError):
        losses.smooth_target(z)
    with pytest.raises(_lib.HipKernelError):
        losses.combined_loss(z.clone().requires_grad_(), z, 48.0)
    with pytest.raises(_lib.HipKernelError):
        losses.gradient_aware_loss2(z, z, "cpu")
    with pytest.raises(_lib.HipKernelError):
        losses.masked_smooth_l1(z, z, 48.0)


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (2, 9), (17, 70), (6, 5)], ids=lambda s: "x".join(map(str, s)))
def test_the_median_judges_agree(shape):
    rng = np.random.default_rng(3)
    for x in ((20 * rng.standard_normal(shape)).astype(np.float32),
              rng.integers(0, 3, shape).astype(np.float32)):      # ties
        once = loss_judge.median5_sort(x)
        assert once.shape == x.shape and once.dtype == np.float32
        assert np.array_equal(once, loss_judge.median5_scipy(x))
        twice = loss_judge.median_blur(x[None], 2)[0]
        assert np.array_equal(twice, loss_judge.median5_scipy(loss_judge.median5_scipy(x)))


def test_the_two_pass_forms_differ():
    """What the GPU test's (2, 17, 70) case can see: the valid median of the input replicated
    four wide is another function than the median of the median."""
    x = (20 * np.random.default_rng(5).standard_normal((2, 17, 70))).astype(np.float32)
    assert int((loss_judge.median_twice_of_wide_replicate(x) != loss_judge.median_blur(x, 2)).sum()) > 0


def test_the_loss_judge_is_the_reference_expression():
    """On a hand-made case: one position, pred a ramp in x, target flat."""
    pred = torch.tensor([[[0., 1., 2.], [0., 1., 2.], [0., 1., 2.]]])
    target = torch.full((1, 3, 3), 1.0)
    direct, edge, comb, grad = loss_judge.torch_loss(pred, target, target, 48.0, 0.5, torch.float64)
    assert direct == pytest.approx((0.5 + 0 + 0.5) * 3 / 9)   # |d| = 1 takes the linear branch: 0.5
    assert edge == pytest.approx(8.0)                          # Sx = 8, Sy = 0, exp(0) = 1
    assert comb == pytest.approx(direct + 0.5 * edge)
    want_edge = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64)
    want_direct = torch.tensor([[-1., 0., 1.]] * 3, dtype=torch.float64) / 9
    assert torch.allclose(grad[0], want_direct + 0.5 * want_edge)


@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="needs make and hipcc")
def test_loss_argument_checks_under_asan():
    """`make asan` runs the four stand-alone drivers; the loss entries' prints its own OK line."""
    r = subprocess.run(["make", "-s", "-j8", "asan"], cwd=REPO, capture_output=True, text=True, timeout=1200)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "OK loss: 0 failed checks" in r.stdout, tail
    assert "AddressSanitizer" not in r.stderr, tail
