"""lea_conv3d_wino44_set_tile / lea_conv3d_wino44_tile (the F(4,3) x F(4,3) tile's geometry:
32 x 2 or 16 x 4, route() in csrc/conv3d_wino.hip) through the query and the setter alone: nothing
launches."""
import pytest

from leastereo_amd import _lib

INVALID = 1001

C2_L0, C2_L1, C2_L2 = (64, 192, 320), (32, 96, 160), (16, 48, 80)
C5_L0, C5_L1, C5_L2 = (88, 336, 504), (44, 168, 252), (22, 84, 126)
# (cin, cout) of the layers the planner puts on this tile, per level
LAYERS = {0: ((32, 32), (8, 24)), 1: ((128, 64), (16, 32)), 2: ((32, 96), (32, 32))}
# the shapes of tests/test_down2_cpu.py
DOWN2 = ((1, 32, 32, 64, 192, 320), (1, 32, 32, 88, 336, 504), (2, 32, 32, 16, 32, 64))


@pytest.fixture
def lib():
    with _lib.tuning(lea_conv3d_wino44_set_tile=None):  # (the tests call the setter themselves)
        yield _lib.load()


def test_setter_takes_auto_and_the_two_widths_only(lib):
    for keep in (16, 32, -1):
        assert lib.lea_conv3d_wino44_set_tile(keep) == 0
        before = lib.lea_conv3d_wino44_tile(1, 32, 32, *C2_L2)
        for bad in (-2, 0, 8, 64):
            assert lib.lea_conv3d_wino44_set_tile(bad) == INVALID, bad
            assert b"lea_conv3d_wino44_set_tile" in lib.lea_last_error()
            assert lib.lea_conv3d_wino44_tile(1, 32, 32, *C2_L2) == before, (keep, bad)
        if keep > 0:
            assert before == keep


def test_auto_rule_on_the_benchmark_shapes(lib):
    """Auto: the narrow tile on C2's quarter-resolution volumes (W = 80: 2.5 wide tiles), the wide
    one on every other C2 shape and on C5's full- and half-resolution ones.  C5's
    quarter-resolution rows (W = 126) are not whole 16-byte blocks: not this tile's layers."""
    assert lib.lea_conv3d_wino44_set_tile(-1) == 0
    assert lib.lea_conv3d_wino44_tile(1, 32, 32, 16, 48, 80) == 16
    assert lib.lea_conv3d_wino44_tile(1, 32, 96, 16, 48, 80) == 16
    for level, vol in ((0, C2_L0), (1, C2_L1)):
        for cin, cout in LAYERS[level]:
            assert lib.lea_conv3d_wino44_tile(1, cin, cout, *vol) == 32, (cin, cout, vol)
    for level, vol in ((0, C5_L0), (1, C5_L1)):
        for cin, cout in LAYERS[level]:
            assert lib.lea_conv3d_wino44_tile(1, cin, cout, *vol) == 32, (cin, cout, vol)
    for cin, cout in LAYERS[2]:
        assert lib.lea_conv3d_wino44_tile(1, cin, cout, *C5_L2) == 0


def test_forced_tiles_and_shapes_off_the_tile(lib):
    for tile in (16, 32):
        assert lib.lea_conv3d_wino44_set_tile(tile) == 0
        for vols in ((C2_L0, C2_L1, C2_L2), (C5_L0, C5_L1)):
            for level, vol in enumerate(vols):
                for cin, cout in LAYERS[level]:
                    assert lib.lea_conv3d_wino44_tile(1, cin, cout, *vol) == tile
        # 16-cout and 8-cout layers run on other tiles; bad shapes answer 0 too
        assert lib.lea_conv3d_wino44_tile(1, 16, 16, *C2_L1) == 0
        assert lib.lea_conv3d_wino44_tile(1, 8, 8, *C2_L0) == 0
        assert lib.lea_conv3d_wino44_tile(1, 30, 32, *C2_L2) == 0
        assert lib.lea_conv3d_wino44_tile(0, 32, 32, *C2_L2) == 0
    # the narrow geometry is built for the default form only
    with _lib.tuning(lea_conv3d_wino44_set_upre=1):
        assert lib.lea_conv3d_wino44_tile(1, 32, 32, *C2_L2) == 32
    with _lib.tuning(lea_conv3d_wino44_set_upre=0, lea_conv3d_wino44_set_sched=1):
        assert lib.lea_conv3d_wino44_tile(1, 32, 32, *C2_L2) == 32
    # the two-barrier tile takes the layers with lea_conv3d_wino44_set(0): not this tile's
    with _lib.tuning(lea_conv3d_wino44_set=0):
        assert lib.lea_conv3d_wino44_tile(1, 32, 32, *C2_L2) == 0


def test_names_and_down2_answers_do_not_depend_on_the_tile(lib):
    answers = {}
    for tile in (-1, 16, 32):
        assert lib.lea_conv3d_wino44_set_tile(tile) == 0
        got = []
        for s in DOWN2:
            got += [lib.lea_conv3d_wino_kernel_name(*s, 0), lib.lea_conv3d_wino_down2_supported(*s),
                    lib.lea_conv3d_wino_down2_kernel_name(*s),
                    lib.lea_conv3d_wino_down2_cat_supported(s[0], 2 * s[1], s[1], *s[2:]),
                    lib.lea_conv3d_wino_down2_cat_kernel_name(s[0], 2 * s[1], s[1], *s[2:]),
                    lib.lea_conv3d_wino_dp_down2_supported(s[0], 8, 8, *s[3:]),
                    lib.lea_conv3d_wino_dp_down2_kernel_name(s[0], 8, 8, *s[3:], 0)]
        for vol in (C2_L2, C5_L2):
            got += [lib.lea_conv3d_wino_kernel_name(1, 32, 32, *vol, 0), lib.lea_conv3d_wino_kernel_name(1, 32, 96, *vol, 0)]
        answers[tile] = got
    assert answers[16] == answers[-1] and answers[32] == answers[-1]
    assert answers[-1][0] == b"conv3d_wino44_kernel" and answers[-1][1] == 1
    assert answers[-1][2] == b"conv3d_wino44_down2_kernel" and answers[-1][3] == 1
    assert answers[-1][4] == b"conv3d_wino44_down2_cat_kernel" and answers[-1][5] == 1
    assert answers[-1][-3] == b"conv3d_wino44_kernel"  # (C2 quarter resolution, 32 -> 96)


def test_env_default_is_registered():
    assert _lib.TUNING_ENV["LEASTEREO_WINO44_TILE"] == "lea_conv3d_wino44_set_tile"


def test_bank_maps_of_both_geometries_are_conflict_free():
    """tools/w44_banks.py, exhaustively: the V-pass's halo reads both as ds_read_b64 and as the
    ds_read2_b64 the compiler pairs a0 / a1 into, its ds_write_b128 and the steps' ds_read_b128,
    every plane, kh, x-half and offset -- 0 extra LDS cycles, and the V-pass map covers every
    (group, channel, row, x-half) with a wave-uniform x-half."""
    from tools import w44_banks
    for q in (8, 4):
        assert w44_banks.check(w44_banks.Geo(q)) == (0, 0, 0), q
