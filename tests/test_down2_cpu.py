"""The stems' down-sampling epilogues, checked without a GPU: the index claim they rest on, the
two new entries' argument checks (nothing launches on a refused call: the return code comes
from the host checks), the binding, and the executor's fused route as graph logic on CPU
float64 (torch stand-ins for the launches, as tests/test_executor_plan_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from leastereo_amd import _lib
from leastereo_amd import executor as ex
from leastereo_amd import kernels
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from leastereo_amd.weights import synthetic_state_dict
from oracle import torch_ref as ref
from tests.executor_stands import Stand, _act
from tests.golden_util import arch, normal
from tests.test_capi import declared_symbols

INVALID, UNSUPPORTED = 1001, 1002


def _axis_index_f32(n_in, n_out):
    """common.h axis_ratio / axis_index (align_corners) in float32, for every output index."""
    f = np.float32
    ratio = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    real = ratio * np.arange(n_out, dtype=np.float32)
    assert real.dtype == np.float32
    i0 = np.minimum(np.floor(real).astype(np.int64), n_in - 1)
    lam = np.clip(real - i0.astype(np.float32), f(0), f(1))
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, lam


def test_halving_reads_one_aligned_pair_per_output():
    """in == 2 out: both source indices of output o are in {2o, 2o + 1}, for every out in
    1..1024 -- the down-sampling is an aligned 2 x 2 x 2 reduction.  Only the last index ever
    starts at 2o + 1 (then i1 == i0 and the weight of i1 need not be 0)."""
    for n_out in range(1, 1025):
        i0, i1, lam = _axis_index_f32(2 * n_out, n_out)
        o = np.arange(n_out)
        assert ((i0 == 2 * o) | (i0 == 2 * o + 1)).all(), n_out
        assert ((i1 == 2 * o) | (i1 == 2 * o + 1)).all(), n_out
        odd = np.nonzero(i0 == 2 * o + 1)[0]
        assert set(odd) <= {n_out - 1}, (n_out, odd)
        assert (i1[odd] == i0[odd]).all()
    i0, i1, lam = _axis_index_f32(192, 96)
    assert i0[-1] == 191 and lam[-1] > 0  # real = 191.00002


def test_binding_declares_the_new_entries():
    lib = _lib.load()
    assert lib.lea_abi_version() == _lib.ABI_VERSION == 14  # additive: the ABI number stays
    new = {"lea_cv_stem_combine_down2": 18, "lea_cv_stem_down2_supported": 5,
           "lea_conv3d_bnrelu_wino_down2": 16, "lea_conv3d_wino_down2_supported": 6,
           "lea_conv3d_wino_down2_kernel_name": 6}
    declared = declared_symbols()
    for name, nargs in new.items():
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["lea_conv3d_wino_down2_kernel_name"][0] is ctypes.c_char_p
    assert _lib.SIGNATURES["lea_cv_stem_combine_down2"][1][9] is ctypes.c_int64  # y2's batch stride


def test_cv_stem_down2_argument_checks():
    lib = _lib.load()
    m, y, y2 = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)

    def call(lm=m, rm=m, scale=None, shift=None, y=y, y2=y2, d3=4, h=4, w=8, flags=1, dtype=0, ybs=0, y2bs=0):
        return lib.lea_cv_stem_combine_down2(lm, 0, rm, 0, scale, shift, y, ybs, y2, y2bs, 1, 16, d3, h, w, flags,
                                             dtype, None)

    for kw in ({"lm": None}, {"rm": None}, {"y": None}, {"y2": None}):
        assert call(**kw) == INVALID and b"null" in lib.lea_last_error(), kw
    assert call(scale=m) == INVALID  # scale without shift
    assert call(flags=1 | 64) == INVALID and b"unknown flag" in lib.lea_last_error()
    assert call(flags=1 | _lib.LEA_PAIR_SUM) == UNSUPPORTED
    assert call(flags=0x100) == INVALID  # the plain entry's probe variants are not taken here
    for kw in ({"d3": 5}, {"h": 3}, {"w": 6}, {"w": 10}, {"d3": 566}, {"dtype": _lib.LEA_BF16}):
        assert call(**kw) == UNSUPPORTED, kw
        assert not lib.lea_cv_stem_down2_supported(16, kw.get("d3", 4), kw.get("h", 4), kw.get("w", 8),
                                                   kw.get("dtype", 0))
    assert call(y2=ctypes.c_void_p((3 << 20) + 4)) == INVALID and b"alignment" in lib.lea_last_error()
    assert call(y2=ctypes.c_void_p((2 << 20) + 64)) == INVALID and b"overlap" in lib.lea_last_error()
    # the benchmark's shapes are taken: C2 (D3 = 64), C5 (D3 = 88), the golden e2e case (D3 = 16)
    for d3, h, w in ((64, 192, 320), (88, 336, 504), (16, 32, 64)):
        assert lib.lea_cv_stem_down2_supported(32, d3, h, w, 0)
    assert lib.lea_cv_stem_down2_supported(32, 224, 4, 8, 0) and not lib.lea_cv_stem_down2_supported(32, 226, 4, 8, 0)


def test_wino_down2_argument_checks():
    lib = _lib.load()
    x, w, y = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)

    def call(x=x, w=w, scale=None, shift=None, y=y, cin=32, cout=32, d=4, h=2, wd=32, flags=1, dtype=0):
        return lib.lea_conv3d_bnrelu_wino_down2(x, 0, w, scale, shift, y, 0, 1, cin, cout, d, h, wd, flags, dtype,
                                                None)

    for kw in ({"x": None}, {"w": None}, {"y": None}):
        assert call(**kw) == INVALID and b"null" in lib.lea_last_error(), kw
    assert call(scale=w) == INVALID
    for kw in ({"d": 5}, {"h": 3}, {"wd": 30}, {"wd": 34}, {"cin": 30}):
        assert call(**kw) == INVALID, kw
    assert call(y=x) == INVALID and b"aliases" in lib.lea_last_error()
    assert call(y=ctypes.c_void_p((3 << 20) + 8)) == INVALID and b"alignment" in lib.lea_last_error()
    assert call(flags=1 | _lib.LEA_RESIDUAL) == UNSUPPORTED and b"LEA_RESIDUAL" in lib.lea_last_error()
    assert call(flags=1 | _lib.LEA_PAIR_SUM) == UNSUPPORTED
    assert call(flags=1 | 64) == INVALID and b"unknown flag" in lib.lea_last_error()
    assert call(dtype=_lib.LEA_BF16) == UNSUPPORTED
    # only where the planner puts the shape on the F(4,3) x F(4,3) tile
    assert call(cout=16) == UNSUPPORTED and b"planner" in lib.lea_last_error()
    assert not lib.lea_conv3d_wino_down2_supported(1, 32, 16, 4, 2, 32)
    assert lib.lea_conv3d_wino_down2_kernel_name(1, 32, 16, 4, 2, 32) is None
    for shape in ((1, 32, 32, 64, 192, 320), (1, 32, 32, 88, 336, 504), (2, 32, 32, 16, 32, 64)):
        assert lib.lea_conv3d_wino_down2_supported(*shape)
        assert lib.lea_conv3d_wino_down2_kernel_name(*shape) == b"conv3d_wino44_down2_kernel"
        # the plain form's reported name is what it was
        assert lib.lea_conv3d_wino_kernel_name(shape[0], shape[1], shape[2], *shape[3:], 0) == b"conv3d_wino44_kernel"
    # another tile or instantiation of the plain form: no DOWN form beside it
    for setter, v in (("lea_conv3d_wino44_set", 0), ("lea_conv3d_wino44_set_upre", 1),
                      ("lea_conv3d_wino44_set_sched", 1)):
        with _lib.tuning(**{setter: v}):
            assert not lib.lea_conv3d_wino_down2_supported(1, 32, 32, 64, 192, 320), setter
            assert call() == UNSUPPORTED, setter


def test_supported_helpers_are_false_off_the_device():
    """CPU tensors never take the fused route (tests/test_executor_plan_cpu.py relies on it)."""
    assert not kernels.cv_stem_down2_supported(torch.zeros(1, 288, 1, 32, 64), 32, 16)
    assert not kernels.conv3d_wino_down2_supported(torch.zeros(1, 32, 16, 32, 64), 32)
    assert not kernels.conv3d_wino_down2_supported(torch.zeros(1, 32, 16, 32, 64, dtype=torch.float64), 32)


# ------------------------------------------------------------ the executor's fused route
class FakeDown(Stand):
    """+ stand-ins for the two down-sampling launches: the plain launch, then F.interpolate."""

    @staticmethod
    def _half(y):
        return F.interpolate(y, size=tuple(n // 2 for n in y.shape[2:]), mode="trilinear", align_corners=True)

    def conv3d_bnrelu_wino_down2(self, x, packed, cout, scale, shift, relu=True):
        self.log.append(("wino_down2",))
        return self._half(_act(F.conv3d(x, packed.to(x.dtype), padding=1), scale, shift, relu))


@pytest.mark.parametrize("stem0_down", [True, False])
@pytest.mark.parametrize("fused", [True, False])
def test_matching_executor_fused_route_matches_oracle(monkeypatch, fused, stem0_down):
    fk = FakeDown().install(monkeypatch, extra=("conv3d_bnrelu_wino_down2",))
    monkeypatch.setattr(kernels, "conv3d_wino_down2_supported", lambda x, cout: True)
    monkeypatch.setattr(ex, "CV_STEM", False)
    monkeypatch.setattr(ex.MatchingExecutor, "FUSED_DOWN", fused)
    resampled = []
    real_rs = fk.conv3d_bnrelu_resampled
    monkeypatch.setattr(kernels, "conv3d_bnrelu_resampled",
                        lambda x, size, *a, **k: (resampled.append(tuple(x.shape[2:])), real_rs(x, size, *a, **k))[1])
    args = default_arch_args(LEAStereoArgs(maxdisp=48))
    a = arch()
    m = LEAStereo(args, "cpu")
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    m.load_state_dict(sd, strict=True)
    m = m.double().eval()
    me = ex.MatchingExecutor(m.matching)
    assert "cells.0.share" in me.p and m.matching.cells[0].downup_sample < 0
    x = normal(903, (1, 64, 16, 32, 64)).double()  # the e2e case's cost volume (96x192 D48)
    with torch.no_grad():
        stem0 = me.conv("stem0", x)
        # stem0's side output, as lea_cv_stem_combine_down2 hands it over on the fused route
        down = FakeDown._half(stem0) if (stem0_down and fused) else None
        got = me._from_stem0(stem0, down)
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        want = ref.matching_forward(sd64, x, a["net_arch_mat"], a["cell_arch_mat"])
    assert (("wino_down2",) in fk.log) == fused
    # an L0 volume is re-read by a resampling conv only where its producer did not down-sample:
    # the stems' two on today's route, and always cell 11's read of cell 10's output
    l0_rereads = resampled.count((16, 32, 64)) - 1
    assert l0_rereads == (2 if not fused else (0 if stem0_down else 1)), resampled
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), err


def test_fused_route_is_off_with_a_tap(monkeypatch):
    """A stage tap sees stem1 at full resolution: the executor keeps today's launches."""
    fk = FakeDown().install(monkeypatch, extra=("conv3d_bnrelu_wino_down2",))
    monkeypatch.setattr(kernels, "conv3d_wino_down2_supported", lambda x, cout: True)
    monkeypatch.setattr(ex, "CV_STEM", False)
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=48)), "cpu")
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    m.load_state_dict(sd, strict=True)
    m = m.double().eval()
    me = ex.MatchingExecutor(m.matching)
    seen = {}
    me.tap = lambda name, t: seen.setdefault(name, tuple(t.shape))
    with torch.no_grad():
        me.run(normal(903, (1, 64, 16, 32, 64)).double())
    assert ("wino_down2",) not in fk.log
    assert seen["stem1"] == (1, 32, 16, 32, 64)
