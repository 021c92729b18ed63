"""The direct f32 and the bf16 conv planners' answers, recorded from the commit before their route
refactor (tools/wino_routes.py --table conv -> tests/golden/conv_routes.json), recomputed from
the built library: every name query of both engines, lea_conv3d_bf16_pair_supported and the
packed sizes of 360 volumes, the 2D name queries of 120 planes, at the default settings, and a
digest of that table under every single value and every pair of values of the eight routing
hooks.  Host queries only.

Hand corrections of the recording (a query that disagreed with the launch; the launch's rule
holds):
  * A route without an instantiation.  Under lea_conv3d_set_tile_override or
    lea_conv3d_bf16_set_tile_override the parent's name queries could answer a kernel that is
    not instantiated (conv3d_dma_kernel<4, 4, 64, 2, 3, false>, conv_bf16_kernel<3, 2, 2, 16,
    4, 2, true>) while the launch returned LEA_E_UNSUPPORTED.  The recording holds None there
    (wino_routes.conv_fix, from the instantiation lists); the library's own answers are
    compared uncorrected, so a name it gives is always one it can launch.
The queries that already existed answer everything else as before.  The two exports that are new
(the parent could not record them) answer for a launch's whole argument list:
  * lea_conv3d_launch_kernel_name: a resampled 1x1 of more than 128 input channels or of two
    sources runs on the register-staged engine; lea_conv3d_kernel_name, which has no cin,
    keeps answering for cin <= 128.
  * lea_conv3d_launch_kernel_name_bf16: a conv of two sources stays on the tile kernel where
    one source would stream, and LEA_PAIR_SUM names the pair launch's kernel, which
    kernels._pair_kernel_name_bf16 used to restate from an environment variable (PAIR_NAMES is
    its table); lea_conv3d_kernel_name_bf16 is that export with cin2 = 0 and no flags.
They are pinned here by identity with the old queries wherever cin2 = 0, flags = 0 and
cin <= 128."""
import ctypes
import json
import os

import pytest

from leastereo_amd import _lib
from tools import wino_routes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")
CONV = wino_routes.CONV

# what kernels._pair_kernel_name_bf16 answered for the pair launch of two sources of cb channel
# blocks into 8 cb channels, by lea_conv3d_bf16_set_pair_split: PAIR_NAMES[split][cb]
PAIR_NAMES = {
    0: {1: "conv_bf16_stream_kernel<1, 1, 8, 1, 2>", 2: "conv_bf16_stream_kernel<1, 1, 4, 2, 2>"},
    1: {1: "conv_bf16_pair_kernel<8, 1, false>", 2: "conv_bf16_pair_kernel<4, 2, false>"},
    2: {1: "conv_bf16_pair_kernel<8, 1, true>", 2: "conv_bf16_pair_kernel<4, 2, false>"},
    3: {1: "conv_bf16_pair_kernel<8, 1, true>", 2: "conv_bf16_stream_kernel<1, 1, 4, 2, 2>"},
}


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    return wino_routes.record(_lib.load(), CONV)


def test_default_routes(want, got):
    assert len(CONV.shapes) == len(want["default"]) == 480
    assert not wino_routes.moved({**want, "single": {}, "pair": {}}, got, CONV)


@pytest.mark.parametrize("part", ["single", "pair"])
def test_routes_under_every_setting(want, got, part):
    assert set(got[part]) == set(want[part]) and len(want["single"]) == 8
    assert [k for k in want[part] if want[part][k] != got[part][k]] == []


def test_sweep_left_the_hooks_as_found(want, got):
    assert wino_routes.table(_lib.load(), CONV) == [got["rows"][i] for i in got["default"]]


def test_the_recording_was_corrected_somewhere():
    """conv_fix is not vacuous: the issue's two examples are names it removes."""
    assert not wino_routes.instantiated("conv3d_dma_kernel<2, 4, 64, 2, 3, true>")
    assert not wino_routes.instantiated("conv3d_dma_kernel<4, 4, 64, 2, 3, false>")
    assert not wino_routes.instantiated("conv_bf16_kernel<3, 2, 2, 16, 4, 2, true>")
    assert wino_routes.instantiated("conv3d_dma_kernel<2, 4, 64, 2, 3, false>")
    assert wino_routes.instantiated("conv_bf16_kernel<3, 1, 1, 4, 2, 2, false>")


def test_new_exports_equal_the_old_queries():
    lib = _lib.load()
    settings = [{}, {"lea_conv3d_set_rs_gather": 0}, {"lea_conv3d_set_tile_override": (4, 64, 2)},
                {"lea_conv3d_bf16_set_variant": 1}, {"lea_conv3d_bf16_set_stream1x1": 0},
                {"lea_conv3d_bf16_set_tile_override": (16, 4, 2)}]
    for s in settings:
        with _lib.tuning(**s):
            for b, ci, co, *vol in wino_routes.SHAPES:
                for k in (1, 3):
                    for rs in (0, 1):
                        if ci <= 128:
                            assert lib.lea_conv3d_launch_kernel_name(b, ci, 0, co, *vol, k, rs) == \
                                lib.lea_conv3d_kernel_name(b, co, *vol, k, rs), (s, b, ci, co, vol, k, rs)
                    for cv in (0, 1):
                        assert lib.lea_conv3d_launch_kernel_name_bf16(b, ci, 0, co, *vol, k, 0, cv) == \
                            lib.lea_conv3d_kernel_name_bf16(b, co, ci, *vol, k, cv), (s, b, ci, co, vol, k, cv)


def test_new_exports_follow_the_launch():
    lib = _lib.load()
    l2 = (16, 48, 80)
    # resampled 1x1: the gather-GEMM up to 128 input channels of one source
    assert lib.lea_conv3d_kernel_name(1, 64, *l2, 1, 1) == b"conv1x1_rs_f32_kernel<4>"
    assert lib.lea_conv3d_launch_kernel_name(1, 128, 0, 64, *l2, 1, 1) == b"conv1x1_rs_f32_kernel<4>"
    assert lib.lea_conv3d_launch_kernel_name(1, 136, 0, 64, *l2, 1, 1) == b"conv3d_reg_kernel<1, 4, 1, 32, true>"
    assert lib.lea_conv3d_launch_kernel_name(1, 64, 32, 64, *l2, 1, 1) == b"conv3d_reg_kernel<1, 4, 1, 32, true>"
    with _lib.tuning(lea_conv3d_set_rs_gather=0):
        assert lib.lea_conv3d_launch_kernel_name(1, 136, 0, 64, *l2, 1, 1) == lib.lea_conv3d_kernel_name(1, 64, *l2, 1, 1)
    # bf16: two sources of one conv stay on the tile kernel where one source streams
    assert lib.lea_conv3d_kernel_name_bf16(1, 16, 32, *l2, 3, 0) == b"conv_bf16_stream_kernel<1, 1, 4, 2, 2>"
    assert lib.lea_conv3d_launch_kernel_name_bf16(1, 32, 16, 16, *l2, 3, 0, 0) == b"conv_bf16_kernel<3, 1, 1, 4, 2, 2, false>"
    # the pair launch: the table kernels._pair_kernel_name_bf16 encoded
    for split, names in PAIR_NAMES.items():
        with _lib.tuning(lea_conv3d_bf16_set_pair_split=split):
            for cb, name in names.items():
                assert lib.lea_conv3d_launch_kernel_name_bf16(1, 16 * cb, 8 * cb, 8 * cb, 4, 8, 16, 3, _lib.LEA_PAIR_SUM, 0) == \
                    name.encode(), (split, cb)
    # ... except that 8 + 8 -> 16 runs the split-wave kernel's plain tile (run(): cout <= 8 for the paired one)
    assert lib.lea_conv3d_launch_kernel_name_bf16(1, 16, 8, 16, 4, 8, 16, 3, _lib.LEA_PAIR_SUM, 0) == \
        b"conv_bf16_pair_kernel<8, 1, false>"
    # where lea_conv3d_bf16_pair_supported says no, the launch refuses and the query answers NULL
    for shape in [(1, 8, 8, 3, 8, 16), (1, 8, 24, 4, 8, 16), (1, 24, 8, 4, 8, 16)]:
        b, ci, co, *vol = shape
        assert lib.lea_conv3d_bf16_pair_supported(*shape) == 0
        assert lib.lea_conv3d_launch_kernel_name_bf16(b, 2 * ci, ci, co, *vol, 3, _lib.LEA_PAIR_SUM, 0) is None
    with _lib.tuning(lea_conv3d_bf16_set_variant=1):
        assert lib.lea_conv3d_bf16_pair_supported(1, 8, 8, 4, 8, 16) == 0


def test_a_route_without_an_instantiation_is_refused_and_unnamed():
    """Under a tile override that asks for a tile the library does not hold, the name query answers
    NULL with the error set and the launch returns LEA_E_UNSUPPORTED before any launch (1002; dummy
    operands; no GPU is touched); the hooks read back as found."""
    lib = _lib.load()
    x, w, y = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)
    before = [_lib.tuning_get(h) for h in ("lea_conv3d_set_tile_override", "lea_conv3d_bf16_set_tile_override")]
    with _lib.tuning(lea_conv3d_set_tile_override=(4, 64, 2)):
        assert lib.lea_conv3d_costvolume_kernel_name(1, 32, 64, 192, 320) is None
        assert b"no tile" in lib.lea_last_error()
        assert lib.lea_conv3d_kernel_name(1, 64, 64, 192, 320, 3, 0) is None
        assert lib.lea_conv3d_bnrelu_costvolume(x, x, 0, w, None, None, y, 0, 1, 32, 32, 64, 192, 320, 1, _lib.LEA_F32,
                                                None) == 1002
        assert b"no tile <2, 4, 64, 2>" in lib.lea_last_error()
    with _lib.tuning(lea_conv3d_bf16_set_tile_override=(16, 4, 2)):
        assert lib.lea_conv3d_kernel_name_bf16(1, 32, 64, 64, 192, 320, 3, 1) is None
        assert b"no tile" in lib.lea_last_error()
        assert lib.lea_conv3d_bnrelu_costvolume_bf16(x, x, 0, w, None, None, y, 0, 1, 32, 32, 64, 192, 320, 1,
                                                     None) == 1002
        assert b"td=4" in lib.lea_last_error()
    assert [_lib.tuning_get(h) for h in ("lea_conv3d_set_tile_override", "lea_conv3d_bf16_set_tile_override")] == before
    assert lib.lea_conv3d_costvolume_kernel_name(1, 32, 64, 192, 320) == b"conv3d_dma_kernel<2, 2, 16, 2, 3, true>"
