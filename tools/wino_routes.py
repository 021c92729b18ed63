#!/usr/bin/env python
"""Record what a conv planner answers for a fixed list of shapes (host queries only, no GPU) -- at
the default settings as a full table, and as a digest of that table for every single tuning value
and every pair of values of two different routing hooks.  Two tables:

  wino  the f32 Winograd planner: the kernel names, the F(4,3) x F(4,3) geometry, the down-sampling
        queries and the packed size
  conv  the direct f32 and the bf16 planners: every name query, lea_conv3d_bf16_pair_supported and
        the packed sizes, plus the 2D name queries of four plane sizes

    python tools/wino_routes.py --write tests/golden/wino_routes.json   # record (from the parent)
    python tools/wino_routes.py --check tests/golden/wino_routes.json   # compare
    python tools/wino_routes.py --table conv --write tests/golden/conv_routes.json

tests/test_wino_routes_cpu.py and tests/test_conv_routes_cpu.py run the comparison: a refactor of a
planner must leave them green.
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import itertools
import json
import os
import re
import sys
from typing import NamedTuple

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leastereo_amd import _lib  # noqa: E402

BATCHES = (1, 8)
CHANNELS = ((8, 8), (8, 24), (16, 16), (16, 32), (32, 32), (32, 96), (32, 64), (64, 64), (128, 64), (32, 48),
            (64, 32), (8, 4), (16, 5), (12, 16), (32, 288))
VOLUMES = ((64, 192, 320), (32, 96, 160), (16, 48, 80), (88, 336, 504), (44, 168, 252), (22, 84, 126),
           (16, 32, 64), (6, 5, 68), (4, 2, 32), (5, 7, 66), (16, 32, 16), (2, 2, 4))
SHAPES = [(b, ci, co) + v for b in BATCHES for ci, co in CHANNELS for v in VOLUMES]

# hook -> (the values swept, the header's default: used to put the hook back only on a library
# that predates lea_tuning_get)
SWEEP = {
    "lea_conv3d_wino_set_w22": (range(3), 0),
    "lea_conv3d_wino_set_variant": (range(8), 0),
    "lea_conv3d_wino2_set_walk": ((0, 1, 4), 0),
    "lea_conv3d_wino2_set_halo16": (range(2), 1),
    "lea_conv3d_wino2_set_lane_halo16": (range(3), 2),
    "lea_conv3d_wino_set_fence": (range(2), 1),
    "lea_conv3d_wino2_set_pipeline": (range(2), 1),
    "lea_conv3d_wino2p_set_wpre": (range(2), 1),
    "lea_conv3d_wino44_set": (range(4), 2),
    "lea_conv3d_wino44_set_upre": (range(2), 0),
    "lea_conv3d_wino44_set_sched": (range(4), 0),
    "lea_conv3d_wino44_set_tile": ((-1, 16, 32), -1),
    "lea_conv3d_wino_set_epi_buf": (range(2), 1),
    "lea_conv3d_wino_set_small_cout": (range(2), 0),
    "lea_conv3d_wino_set_block48": (range(2), 1),
    "lea_conv3d_wino_set_tile_override": (((1, 1, 2), (1, 2, 4), (2, 2, 2), (1, 2, 8)), (0, 0, 0)),
}
# swept alone only: the workgroup order changes no route
SINGLE_ONLY = {"lea_conv3d_wino44_set_group": (range(-1, 17), -1)}


def _s(p):
    return p.decode() if p else None


def row(lib, b, ci, co, d, h, w):
    s = (b, ci, co, d, h, w)
    return [_s(lib.lea_conv3d_wino_kernel_name(*s, 0)), _s(lib.lea_conv3d_wino_kernel_name(*s, 1)),
            lib.lea_conv3d_wino44_tile(*s),
            lib.lea_conv3d_wino_dp_down2_supported(*s),
            _s(lib.lea_conv3d_wino_dp_down2_kernel_name(*s, 0)), _s(lib.lea_conv3d_wino_dp_down2_kernel_name(*s, 1)),
            lib.lea_conv3d_wino_down2_supported(*s), _s(lib.lea_conv3d_wino_down2_kernel_name(*s)),
            lib.lea_conv3d_wino_down2_cat_supported(b, ci, 4, co, d, h, w),
            _s(lib.lea_conv3d_wino_down2_cat_kernel_name(b, ci, 4, co, d, h, w)),
            lib.lea_conv3d_wino_packed_floats(co, ci)]


class Table(NamedTuple):
    shapes: list
    row: object        # (lib, *shape) -> the list of answers
    sweep: dict        # hook -> (the values swept alone and in pairs, the header's default)
    single_only: dict  # hooks swept alone only
    fix: object = None  # the hand corrections applied to a recording (None: none)


WINO = Table(SHAPES, row, SWEEP, SINGLE_ONLY)

# ---- the direct f32 and the bf16 planners
PLANES = ((192, 320), (96, 160), (48, 80), (5, 17))
CONV_SHAPES = SHAPES + [(b, ci, co) + p for b in BATCHES for ci, co in CHANNELS for p in PLANES]
CONV_SWEEP = {
    "lea_conv3d_set_tile_override": (((2, 16, 2), (1, 16, 1), (4, 64, 2), (8, 32, 1), (2, 64, 2)), (0, 0, 0)),
    "lea_conv3d_set_rs_gather": (range(2), 1),
    "lea_conv1x1_set_vector": (range(2), 1),
    "lea_conv2d_set_small": (range(2), 1),
    "lea_conv3d_bf16_set_tile_override": (((16, 4, 2), (8, 2, 1), (4, 1, 2), (16, 2, 1)), (0, 0, 0)),
    "lea_conv3d_bf16_set_variant": (range(2), 0),
    "lea_conv3d_bf16_set_stream1x1": (range(2), 1),
    "lea_conv3d_bf16_set_pair_split": (range(4), 3),
}


def conv_row(lib, b, ci, co, *vol):
    if len(vol) == 2:
        return [_s(lib.lea_conv2d_kernel_name(b, co, *vol)), _s(lib.lea_conv2d_kernel_name_cin(b, ci, co, *vol))]
    s = (b, co) + vol
    return [_s(lib.lea_conv3d_kernel_name(*s, 3, 0)), _s(lib.lea_conv3d_kernel_name(*s, 1, 0)),
            _s(lib.lea_conv3d_kernel_name(*s, 3, 1)), _s(lib.lea_conv3d_kernel_name(*s, 1, 1)),
            _s(lib.lea_conv3d_costvolume_kernel_name(*s)), _s(lib.lea_conv1x1_heads_kernel_name(*s)),
            _s(lib.lea_conv3d_kernel_name_bf16(b, co, ci, *vol, 3, 0)), _s(lib.lea_conv3d_kernel_name_bf16(b, co, ci, *vol, 1, 0)),
            _s(lib.lea_conv3d_kernel_name_bf16(b, co, ci, *vol, 3, 1)),
            lib.lea_conv3d_bf16_pair_supported(b, ci, co, *vol),
            lib.lea_conv3d_packed_floats(co, ci, 3), lib.lea_conv3d_packed_floats(co, ci, 1),
            lib.lea_conv3d_packed_elems_bf16(co, ci, 3), lib.lea_conv3d_packed_elems_bf16(co, ci, 1)]


def instantiated(name):
    """Whether a DMA-engine or bf16 tile name is a kernel the library holds (the lists of
    conv3d_impl.h and conv3d_bf16.hip run()); every other name: True."""
    m = re.fullmatch(r"conv3d_dma_kernel<(\d), (\d), (\d+), (\d), (\d), (true|false)>", name)
    if m:
        mt, nt, tw, td, kd = (int(v) for v in m.groups()[:5])
        if m.group(6) == "true" or kd != 3:  # the cost-volume, 2D and depth-paired tiles
            return nt <= 2 and tw == 16 and (td == 1 or kd == 3)
        return ((tw > 16 or nt <= 2) and mt * nt * td <= 16 and (mt, nt, td) not in ((1, 8, 2), (2, 8, 1), (4, 4, 1))
                and (mt, nt, tw, td) != (4, 2, 64, 2))
    m = re.fullmatch(r"conv_bf16_kernel<(\d), (\d), (\d), (\d+), (\d), (\d), (true|false)>", name)
    if m:
        ks, mt, wc, th, td, nb = (int(v) for v in m.groups()[:6])
        tiles = ((3, 2, 2), (3, 1, 2)) if m.group(7) == "true" else \
            ((3, 2, 1), (3, 2, 2), (3, 1, 1), (3, 1, 2), (3, 4, 1), (3, 4, 2), (1, 1, 4))
        return (mt, wc) in ((1, 1), (2, 1), (1, 2), (2, 2), (1, 4)) and (ks, td, nb) in tiles
    return True


def conv_fix(r):
    """The hand correction of a recording: a tile override can make a name query of the parent
    answer a kernel that is not instantiated (the launch refuses); the answer is NULL."""
    return [None if isinstance(v, str) and not instantiated(v) else v for v in r]


CONV = Table(CONV_SHAPES, conv_row, CONV_SWEEP, {}, conv_fix)
TABLES = {"wino": WINO, "conv": CONV}


def table(lib, t=WINO, fix=False):
    rows = [t.row(lib, *s) for s in t.shapes]
    return [t.fix(r) for r in rows] if fix and t.fix else rows


def digest(t):
    return hashlib.sha1(json.dumps(t, separators=(",", ":")).encode()).hexdigest()[:8]


@contextlib.contextmanager
def _set(lib, hook, value, default):
    args = value if isinstance(value, tuple) else (value,)
    if hasattr(_lib, "tuning"):
        with _lib.tuning(**{hook: value}):
            yield
        return
    _lib.check(getattr(lib, hook)(*args), hook)
    try:
        yield
    finally:
        _lib.check(getattr(lib, hook)(*(default if isinstance(default, tuple) else (default,))), hook)


def record(lib, tab=WINO, fix=False):
    """{"shapes": digest of the shapes, "rows": the distinct rows of the default table, "default":
    each shape's index into them, "single": {hook: [digest per value]}, "pair": {"hook1 hook2":
    [[digest per value of hook2] per value of hook1]}}; fix: with the table's hand corrections (a
    recording from the parent library)"""
    t = table(lib, tab, fix)
    rows = [r for i, r in enumerate(t) if r not in t[:i]]
    out = {"shapes": digest([list(s) for s in tab.shapes]), "rows": rows, "default": [rows.index(r) for r in t],
           "single": {}, "pair": {}}
    for hook, (values, default) in {**tab.sweep, **tab.single_only}.items():
        out["single"][hook] = []
        for v in values:
            with _set(lib, hook, v, default):
                out["single"][hook].append(digest(table(lib, tab, fix)))
    for (h1, (v1s, d1)), (h2, (v2s, d2)) in itertools.combinations(tab.sweep.items(), 2):
        grid = out["pair"][h1 + " " + h2] = []
        for v1 in v1s:
            with _set(lib, h1, v1, d1):
                grid.append([])
                for v2 in v2s:
                    with _set(lib, h2, v2, d2):
                        grid[-1].append(digest(table(lib, tab, fix)))
    return out


def moved(want, got, tab=WINO):
    """What differs between two records, as short texts."""
    bad = [] if want["shapes"] == got["shapes"] else ["the list of shapes"]
    for s, w, g in zip(tab.shapes, want["default"], got["default"]):
        if want["rows"][w] != got["rows"][g]:
            bad.append(f"{s}: {want['rows'][w]} -> {got['rows'][g]}")
    bad += [f"{part} {k}" for part in ("single", "pair") for k in want[part] if want[part][k] != got[part].get(k)]
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--write", metavar="JSON")
    g.add_argument("--check", metavar="JSON")
    ap.add_argument("--table", choices=sorted(TABLES), default="wino")
    a = ap.parse_args()
    got = record(_lib.load(), TABLES[a.table], fix=bool(a.write))
    if a.write:
        with open(a.write, "w") as f:  # one line per part
            f.write("{" + ",\n".join(f'"{k}":' + json.dumps(v, separators=(",", ":")) for k, v in got.items()) + "}\n")
        print(f"{a.write}: {len(got['default'])} shapes, {len(got['rows'])} distinct rows, "
              f"{sum(map(len, got['single'].values()))} single settings, "
              f"{sum(len(r) for g_ in got['pair'].values() for r in g_)} pairs")
        return 0
    with open(a.check) as f:
        bad = moved(json.load(f), got, TABLES[a.table])
    print("\n".join(bad[:40]) if bad else "all routes as recorded")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
