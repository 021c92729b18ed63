#!/usr/bin/env python
"""Record what the f32 Winograd planner answers for a fixed list of shapes (host queries only,
no GPU): the kernel names, the F(4,3) x F(4,3) geometry, the down-sampling queries and the packed
size -- at the default settings as a full table, and as a digest of that table for every single
tuning value and every pair of values of two different Winograd hooks.

    python tools/wino_routes.py --write tests/golden/wino_routes.json   # record (from the parent)
    python tools/wino_routes.py --check tests/golden/wino_routes.json   # compare

tests/test_wino_routes_cpu.py runs the comparison: a refactor of the planner must leave it green.
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import itertools
import json
import os
import sys

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


def table(lib):
    return [row(lib, *s) for s in SHAPES]


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


def record(lib):
    """{"shapes": digest of SHAPES, "rows": the distinct rows of the default table, "default": each
    shape's index into them, "single": {hook: [digest per value]}, "pair": {"hook1 hook2": [[digest
    per value of hook2] per value of hook1]}}"""
    t = table(lib)
    rows = [r for i, r in enumerate(t) if r not in t[:i]]
    out = {"shapes": digest([list(s) for s in SHAPES]), "rows": rows, "default": [rows.index(r) for r in t],
           "single": {}, "pair": {}}
    for hook, (values, default) in {**SWEEP, **SINGLE_ONLY}.items():
        out["single"][hook] = []
        for v in values:
            with _set(lib, hook, v, default):
                out["single"][hook].append(digest(table(lib)))
    for (h1, (v1s, d1)), (h2, (v2s, d2)) in itertools.combinations(SWEEP.items(), 2):
        grid = out["pair"][h1 + " " + h2] = []
        for v1 in v1s:
            with _set(lib, h1, v1, d1):
                grid.append([])
                for v2 in v2s:
                    with _set(lib, h2, v2, d2):
                        grid[-1].append(digest(table(lib)))
    return out


def moved(want, got):
    """What differs between two records, as short texts."""
    bad = [] if want["shapes"] == got["shapes"] else ["the list of shapes"]
    for s, w, g in zip(SHAPES, want["default"], got["default"]):
        if want["rows"][w] != got["rows"][g]:
            bad.append(f"{s}: {want['rows'][w]} -> {got['rows'][g]}")
    bad += [f"{part} {k}" for part in ("single", "pair") for k in want[part] if want[part][k] != got[part].get(k)]
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--write", metavar="JSON")
    g.add_argument("--check", metavar="JSON")
    a = ap.parse_args()
    got = record(_lib.load())
    if a.write:
        with open(a.write, "w") as f:  # one line per part
            f.write("{" + ",\n".join(f'"{k}":' + json.dumps(v, separators=(",", ":")) for k, v in got.items()) + "}\n")
        print(f"{a.write}: {len(got['default'])} shapes, {len(got['rows'])} distinct rows, "
              f"{sum(map(len, got['single'].values()))} single settings, "
              f"{sum(len(r) for g_ in got['pair'].values() for r in g_)} pairs")
        return 0
    with open(a.check) as f:
        bad = moved(json.load(f), got)
    print("\n".join(bad[:40]) if bad else "all routes as recorded")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
