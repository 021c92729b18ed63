"""CPU checks of the down-sampling route inside the matching net's cell chain
(MatchingExecutor.FUSED_DOWN_CELLS): which cell's output gets a level-down copy from its own
producers, where conv1 may write cell 5's level itself, how the switch is parsed, and the new
C entries' argument checks (host code only: nothing is launched)."""
import ctypes
import importlib.util
import sys
from types import SimpleNamespace

import pytest
import torch

from leastereo_amd import _lib
from leastereo_amd import executor as ex
from leastereo_amd import kernels
from tests.test_capi import declared_symbols

INVALID, UNSUPPORTED = 1001, 1002
PLAN = [[(0, 0), (1, 1)], [(2, 1), (3, 2)], [(4, 1), (5, 3)]]  # the shipped matching genotype's steps


def _cell(c_out, downup, plan=PLAN, kinds=("conv",) * 6, dims=3):
    return SimpleNamespace(c_out=c_out, downup_sample=downup, steps=len(plan), block_multiplier=4, plan=plan,
                           op_kinds=list(kinds), dims=dims)


def _stub(cells, cls=ex.MatchingExecutor, share=(), wino=True, k=1):
    """An executor over stub cells: only what the routing predicates read."""
    me = object.__new__(cls)
    me.m = SimpleNamespace(cells=cells)
    me.p = {}
    for i, cell in enumerate(cells):
        me.p[f"cells.{i}.preprocess"] = SimpleNamespace(k=k)
        for op in range(len(cell.op_kinds)):
            me.p[f"cells.{i}._ops.{op}"] = SimpleNamespace(wino=object() if wino else None)
    for i in share:
        me.p[f"cells.{i}.share"] = SimpleNamespace(k=1)
    me.s1_group = {i: [(0, 1), (1, 2), (2, 4)] for i in range(len(cells))}
    me.pair_steps, me.s0_pair = {}, {}
    return me


def _twelve():
    """The matching net's level changes: ... cell 10 up to L0, cell 11 (the last) down to L1."""
    downup = [-1, 0, -1, 0, 1, -1, 0, 0, 1, 0, 1, -1]
    chans = [16, 16, 32, 32, 16, 32, 32, 32, 16, 16, 8, 16]
    return [_cell(c, d) for c, d in zip(chans, downup)]


SIZE = (16, 32, 64)


def test_only_the_cell_before_the_last_gets_a_down_tensor():
    me = _stub(_twelve(), share=(0, 5))
    takes = [i for i in range(12) if me._cell_output_takes_down(i, SIZE)]
    assert takes == [10]
    # the finishing launch of a step is its op that is not in the s1 sibling group
    assert [me._finishing_op(10, s) for s in range(3)] == [0, 3, 5]
    # the base executor (the feature net's) never does
    assert not ex.CellGraphExecutor._cell_output_takes_down(me, 10, SIZE)


@pytest.mark.parametrize("why,change", [
    ("switch off", lambda me: setattr(me, "FUSED_DOWN_CELLS", False)),
    ("a tap", lambda me: setattr(me, "tap", lambda name, t: None)),
    ("share on the consumer", lambda me: me.p.__setitem__("cells.11.share", SimpleNamespace(k=1))),
    ("share on the producer", lambda me: me.p.__setitem__("cells.10.share", SimpleNamespace(k=1))),
    ("the consumer does not down-sample", lambda me: setattr(me.m.cells[11], "downup_sample", 0)),
    ("s1 is not the commuted up-sampling", lambda me: setattr(me.m.cells[10], "downup_sample", 0)),
    ("a 3x3x3 preprocess", lambda me: setattr(me.p["cells.10.preprocess"], "k", 3)),
    ("a skip term left to add", lambda me: me.m.cells[10].op_kinds.__setitem__(5, "skip")),
    ("a finishing conv off the Winograd engine", lambda me: setattr(me.p["cells.10._ops.3"], "wino", None)),
    ("paired steps", lambda me: me.pair_steps.__setitem__(10, PLAN)),
    ("a 2D cell", lambda me: setattr(me.m.cells[10], "dims", 2)),
])
def test_route_refusals(why, change):
    me = _stub(_twelve(), share=(0, 5))
    assert me._cell_output_takes_down(10, SIZE)
    change(me)
    assert not me._cell_output_takes_down(10, SIZE), why


def test_route_refuses_odd_sizes_and_c8():
    me = _stub(_twelve(), share=(0, 5))
    for size in [(15, 32, 64), (16, 31, 64), (16, 32, 62), (16, 32, 63)]:  # odd D, H; W % 4 != 0; odd W
        assert not me._cell_output_takes_down(10, size), size
    assert me._cell_output_takes_down(10, (2, 2, 4))
    c8 = _stub(_twelve(), cls=ex.MatchingExecutorBF16, share=(0, 5))
    assert not c8._cell_output_takes_down(10, SIZE)
    assert not c8._conv1_takes_down((8, 16, 32))


def test_a_later_reader_keeps_the_full_output():
    # cell 10 of 13: cell 12 would read its output as s0
    cells = _twelve() + [_cell(16, 0)]
    assert not any(_stub(cells, share=(0, 5))._cell_output_takes_down(i, SIZE) for i in range(13))
    # twelve cells whose cell 8 looks like cell 10: conv2 reads outs[8]
    cells = _twelve()
    assert not _stub(cells)._cell_output_takes_down(8, SIZE)
    # a two-cell net: cell 0 up, cell 1 down
    two = [_cell(8, 1), _cell(16, -1)]
    assert _stub(two)._cell_output_takes_down(0, SIZE)


def test_conv1_route_predicate():
    me = _stub(_twelve(), share=(0, 5))
    assert me._conv1_takes_down((8, 16, 32))
    assert not me._conv1_takes_down((8, 15, 32)) and not me._conv1_takes_down((7, 16, 32))
    assert not _stub(_twelve(), share=(0,))._conv1_takes_down((8, 16, 32))   # cell 5 reads conv1 alone: no share memo
    assert not _stub(_twelve()[:11], share=(0, 5))._conv1_takes_down((8, 16, 32))  # no conv1 in another depth
    me.tap = lambda name, t: None
    assert not me._conv1_takes_down((8, 16, 32))
    me.tap, me.FUSED_DOWN_CELLS = None, False
    assert not me._conv1_takes_down((8, 16, 32))
    # independent of the stems' switch
    me.FUSED_DOWN_CELLS, me.FUSED_DOWN = True, False
    assert me._conv1_takes_down((8, 16, 32)) and me._cell_output_takes_down(10, SIZE)


def test_kernel_queries_are_false_off_the_device():
    """CPU tensors never take the routes (the executor-plan tests with stand-in kernels rely on it)."""
    x = torch.zeros(1, 64, 8, 16, 32)
    assert not kernels.conv3d_wino_down2_cat_supported(x, x, 64)
    assert not kernels.conv3d_wino_dp_down2_supported(torch.zeros(1, 8, 64, 192, 320), 8)
    assert not kernels.resample_down2_supported(torch.zeros(1, 8, 4, 4, 8), (8, 8, 16))
    me = _stub(_twelve(), share=(0, 5))
    assert not me._down_kernels_take(torch.zeros(1, 64, 32, 96, 160), 8, (32, 96, 160), (64, 192, 320))


@pytest.mark.parametrize("value,on", [(None, True), ("1", True), ("0", False), ("", True), ("off", True)])
def test_env_switch_is_parsed_as_fused_down_is(monkeypatch, value, on):
    """The switches are read when the module is imported: a second copy of it under the variable."""
    for var in ("LEASTEREO_FUSED_DOWN_CELLS", "LEASTEREO_FUSED_DOWN"):
        if value is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, value)
    name = "leastereo_amd._executor_env_copy"
    spec = importlib.util.spec_from_file_location(name, ex.__file__)
    mod = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, name, mod)
    spec.loader.exec_module(mod)
    assert mod.MatchingExecutor.FUSED_DOWN_CELLS is on
    assert mod.MatchingExecutor.FUSED_DOWN is on
    # one does not move the other
    monkeypatch.setenv("LEASTEREO_FUSED_DOWN", "1")
    monkeypatch.setenv("LEASTEREO_FUSED_DOWN_CELLS", "0")
    spec.loader.exec_module(mod)
    assert mod.MatchingExecutor.FUSED_DOWN and not mod.MatchingExecutor.FUSED_DOWN_CELLS


# ------------------------------------------------------------------ the C entries (host side)
def test_binding_declares_the_new_entries():
    lib = _lib.load()
    assert lib.lea_abi_version() == _lib.ABI_VERSION == 14  # additive: the ABI number stays
    new = {"lea_conv3d_wino_down2_cat_supported": 7, "lea_conv3d_wino_down2_cat_kernel_name": 7,
           "lea_conv3d_bnrelu_wino_down2_cat": 19, "lea_conv3d_wino_dp_down2_supported": 6,
           "lea_conv3d_wino_dp_down2_kernel_name": 7, "lea_conv3d_bnrelu_wino_dp_down2": 20,
           "lea_resample3d_down2_supported": 7, "lea_resample3d_trilinear_down2": 19}
    declared = declared_symbols()
    for name, nargs in new.items():
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


def test_planner_queries_at_the_routed_shapes():
    lib = _lib.load()
    # conv1 (64 + 64 -> 64 at L1) and cell 10's 8 -> 8 ops (L0): C2, C5, the golden e2e case
    for l0 in ((64, 192, 320), (88, 336, 504), (16, 32, 64)):
        l1 = tuple(n // 2 for n in l0)
        assert lib.lea_conv3d_wino_down2_cat_supported(1, 128, 64, 64, *l1)
        assert lib.lea_conv3d_wino_down2_cat_kernel_name(1, 128, 64, 64, *l1) == b"conv3d_wino44_down2_cat_kernel"
        assert lib.lea_conv3d_wino_down2_kernel_name(1, 128, 64, *l1) == b"conv3d_wino44_down2_kernel"
        assert lib.lea_conv3d_wino_dp_down2_supported(1, 8, 8, *l0)
        assert lib.lea_conv3d_wino_dp_down2_kernel_name(1, 8, 8, *l0, 0) == b"conv3d_wino_dp_down2_kernel<16, false>"
        assert lib.lea_conv3d_wino_dp_down2_kernel_name(1, 8, 8, *l0, 1) == b"conv3d_wino_dp_down2_kernel<16, true>"
        assert lib.lea_resample3d_down2_supported(*l1, *l0, 0)
        # the plain launches' names are what they were
        assert lib.lea_conv3d_wino_kernel_name(1, 8, 8, *l0, 0) == b"conv3d_wino_kernel<4, 16, 0, 1, 2, false, true, true>"
    # rows that waste more than a tenth of a 64-wide tile run the 32-wide row pairs
    assert lib.lea_conv3d_wino_dp_down2_kernel_name(2, 8, 8, 6, 4, 96, 0) == b"conv3d_wino_dp_down2_kernel<8, false>"
    for bad in ((1, 8, 8, 5, 4, 64), (1, 8, 8, 4, 3, 64), (1, 8, 8, 4, 4, 66), (1, 8, 16, 4, 4, 64), (1, 6, 8, 4, 4, 64)):
        assert not lib.lea_conv3d_wino_dp_down2_supported(*bad), bad
    assert not lib.lea_conv3d_wino_down2_cat_supported(1, 32, 6, 32, 4, 4, 32)    # a chunk straddles the sources
    assert not lib.lea_conv3d_wino_down2_cat_supported(1, 32, 0, 32, 4, 4, 32)
    assert not lib.lea_conv3d_wino_down2_cat_supported(1, 32, 32, 32, 4, 4, 32)
    # another instantiation of the plain depth-paired launch: no DOWN form beside it
    for setter, v in (("lea_conv3d_wino_set_fence", 0), ("lea_conv3d_wino_set_epi_buf", 0),
                      ("lea_conv3d_wino2_set_halo16", 0), ("lea_conv3d_wino_set_small_cout", 1)):
        with _lib.tuning(**{setter: v}):
            assert not lib.lea_conv3d_wino_dp_down2_supported(1, 8, 8, 64, 192, 320), setter
    assert lib.lea_conv3d_wino_dp_down2_supported(1, 8, 8, 64, 192, 320)
    # down on D; odd D, H; W % 4 != 0; rows of three planes that do not fit the LDS
    for bad in ((4, 4, 8, 2, 8, 16), (4, 4, 8, 7, 8, 16), (4, 4, 8, 8, 7, 16), (4, 4, 8, 8, 8, 18), (4, 4, 8, 8, 8, 4096)):
        assert not lib.lea_resample3d_down2_supported(*bad, 0), bad
    assert lib.lea_resample3d_down2_supported(4, 4, 8, 8, 8, 16, 0) and lib.lea_resample3d_down2_supported(4, 9, 8, 4, 4, 16, 0)
    assert not lib.lea_resample3d_down2_supported(4, 4, 8, 8, 8, 16, _lib.LEA_BF16)


def test_new_entries_argument_checks():
    lib = _lib.load()
    x, w, y, y2 = (ctypes.c_void_p(k << 20) for k in (1, 2, 3, 4))

    def dp(x=x, w=w, scale=None, res=None, y=y, y2=y2, cin=8, cout=8, d=4, h=4, wd=64, flags=1, dtype=0):
        return lib.lea_conv3d_bnrelu_wino_dp_down2(x, 0, w, scale, None, res, 0, y, 0, y2, 0, 1, cin, cout, d, h, wd,
                                                   flags, dtype, None)

    for kw in ({"x": None}, {"w": None}, {"y2": None}):
        assert dp(**kw) == INVALID and b"null" in lib.lea_last_error(), kw
    assert dp(scale=w) == INVALID
    assert dp(flags=1 | _lib.LEA_RESIDUAL) == INVALID and b"without residual" in lib.lea_last_error()
    assert dp(flags=1 | _lib.LEA_PAIR_SUM) == UNSUPPORTED
    assert dp(flags=1 | 64) == INVALID and b"unknown flag" in lib.lea_last_error()
    for kw in ({"d": 5}, {"h": 3}, {"wd": 66}, {"cout": 16}, {"cin": 6}, {"dtype": _lib.LEA_BF16}):
        assert dp(**kw) == UNSUPPORTED, kw
    assert dp(y2=y) == INVALID and b"aliased" in lib.lea_last_error()
    assert dp(y2=ctypes.c_void_p((4 << 20) + 8)) == INVALID and b"alignment" in lib.lea_last_error()
    assert dp(x=ctypes.c_void_p((1 << 20) + 4)) == UNSUPPORTED and b"planner" in lib.lea_last_error()

    def cat(x=x, x2=y2, cin2=16, w=w, y=y, cin=32, cout=32, d=4, h=2, wd=32, flags=1, dtype=0):
        return lib.lea_conv3d_bnrelu_wino_down2_cat(x, 0, x2, 0, cin2, w, None, None, y, 0, 1, cin, cout, d, h, wd,
                                                    flags, dtype, None)

    for kw in ({"x": None}, {"x2": None}, {"w": None}, {"y": None}):
        assert cat(**kw) == INVALID and b"null" in lib.lea_last_error(), kw
    for kw in ({"cin2": 0}, {"cin2": 32}, {"cin2": 6}, {"d": 5}, {"h": 3}, {"wd": 30}):
        assert cat(**kw) == INVALID, kw
    assert cat(x2=ctypes.c_void_p((4 << 20) + 4)) == INVALID and b"alignment" in lib.lea_last_error()
    assert cat(y=y2) == INVALID and b"aliases" in lib.lea_last_error()
    assert cat(flags=1 | _lib.LEA_RESIDUAL) == UNSUPPORTED
    assert cat(cout=16) == UNSUPPORTED and b"planner" in lib.lea_last_error()

    def rs(x=x, y=y, y2=y2, up=(8, 8, 16), scale=None, flags=0, dtype=0):
        return lib.lea_resample3d_trilinear_down2(x, 0, y, 0, y2, 0, 1, 2, 4, 4, 8, *up, scale, None, flags, dtype,
                                                  None)

    assert rs(x=None) == INVALID and rs(y2=None) == INVALID and rs(y=x) == INVALID and rs(y2=y) == INVALID
    assert rs(scale=w) == INVALID
    assert rs(flags=2) == INVALID and b"unknown flag" in lib.lea_last_error()
    for kw in ({"up": (2, 8, 16)}, {"up": (8, 7, 16)}, {"up": (8, 8, 18)}, {"dtype": _lib.LEA_BF16}):
        assert rs(**kw) == UNSUPPORTED, kw
    assert rs(y2=ctypes.c_void_p((4 << 20) + 4)) == INVALID and b"alignment" in lib.lea_last_error()
