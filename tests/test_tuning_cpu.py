"""The table of tuning hooks (lea_tuning_get / lea_tuning_name, csrc/common.h) and
_lib.tuning(): every setter of leastereo_hip_tuning.h is registered, reads back what it was set
to, and tuning() puts everything back.  Nothing launches."""
import os
import re
import subprocess
import sys

import pytest

from leastereo_amd import _lib, kernels

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "leastereo_hip_tuning.h")
# the defaults the header documents, as tests/test_capi.py pins them
DOCUMENTED = {"lea_conv3d_wino44_set": 2, "lea_conv3d_wino44_set_group": -1, "lea_conv3d_wino44_set_sched": 0,
              "lea_conv3d_wino44_set_upre": 0, "lea_conv3d_wino2p_set_wpre": 1,
              "lea_disparity_set_register_form": 4}


def snapshot():
    return {name: _lib.tuning_get(name) for name in _lib.tuning_names()}


def test_every_declared_setter_is_registered():
    with open(HEADER) as f:
        declared = set(re.findall(r"(lea_\w*set\w*)\(", f.read())) - {"lea_tuning_get"}
    names = _lib.tuning_names()
    assert len(names) == len(set(names)) == 31
    assert set(names) == declared


def test_get_then_set_changes_nothing():
    lib = _lib.load()
    for name, values in snapshot().items():
        assert len(values) == (3 if name.endswith("_set_tile_override") else 1), name
        assert getattr(lib, name)(*values) == 0, name
        assert _lib.tuning_get(name) == values, name


def test_unknown_name_and_small_capacity():
    lib = _lib.load()
    one = (_lib._i * 3)()
    assert lib.lea_tuning_get(b"lea_no_such_set", one, 3) == -1 and b"lea_no_such_set" in lib.lea_last_error()
    assert lib.lea_tuning_get(b"lea_conv3d_wino44_set", one, 0) == -1 and lib.lea_last_error()
    assert lib.lea_tuning_get(b"lea_conv3d_wino_set_tile_override", one, 2) == -1
    assert lib.lea_tuning_name(-1) is None and lib.lea_tuning_name(31) is None
    with pytest.raises(_lib.HipKernelError):
        _lib.tuning_get("lea_no_such_set")


def test_documented_defaults_in_a_fresh_process():
    """What a process that never called a setter holds (this one may be mid-suite): the header's
    values, or the LEASTEREO_* variable's where one is set for the hook."""
    env_of = {fn: var for var, fn in _lib.TUNING_ENV.items()}
    code = ("from leastereo_amd import _lib; "
            f"print(*[_lib.tuning_get(n)[0] for n in {list(DOCUMENTED)!r}])")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(HEADER)), check=True,
                         capture_output=True, text=True).stdout.split()
    for (name, value), got in zip(DOCUMENTED.items(), out):
        assert int(got) == int(os.environ.get(env_of.get(name, "")) or value), name


def test_tuning_restores_nested_and_after_an_exception():
    before = snapshot()
    with pytest.raises(ZeroDivisionError):
        with _lib.tuning(lea_conv3d_wino44_set=3, lea_conv3d_wino_set_tile_override=(1, 2, 8)):
            assert _lib.tuning_get("lea_conv3d_wino44_set") == (3,)
            assert _lib.tuning_get("lea_conv3d_wino_set_tile_override") == (1, 2, 8)
            with _lib.tuning(lea_conv3d_wino44_set=0, lea_conv3d_wino2_set_walk=4):
                assert _lib.tuning_get("lea_conv3d_wino44_set") == (0,)
                assert _lib.tuning_get("lea_conv3d_wino2_set_walk") == (4,)
            assert _lib.tuning_get("lea_conv3d_wino44_set") == (3,)
            1 // 0
    assert snapshot() == before


def test_tuning_out_of_range_raises_and_changes_nothing():
    before = snapshot()
    with pytest.raises(_lib.HipKernelError, match="lea_conv3d_wino44_set_sched"):
        with _lib.tuning(lea_conv3d_wino44_set=1, lea_conv3d_wino44_set_sched=9):
            raise AssertionError("not reached")
    assert snapshot() == before
    with pytest.raises(_lib.HipKernelError):
        with _lib.tuning(lea_no_such_set=1):
            raise AssertionError("not reached")
    assert snapshot() == before


def test_wino_depth_f2_restores_the_callers_setting():
    with _lib.tuning(lea_conv3d_wino44_set=3):
        with kernels.wino_depth_f2():
            assert _lib.tuning_get("lea_conv3d_wino44_set") == (0,)
        assert _lib.tuning_get("lea_conv3d_wino44_set") == (3,)
