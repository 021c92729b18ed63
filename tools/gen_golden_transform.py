#!/usr/bin/env python3
"""Golden vectors for the training batch transform (lea_train_transform_u8, leastereo_amd/data.py).

Loads the reference's dataloaders/datasets/common.py by path (plain numpy; the package's
__init__ chain is not imported; read-only tree, no bytecode written) and runs its
``set_rgb_layers`` and ``train_transform`` on seeded tiny samples under ``random.seed(s)``,
with a recording ``randint`` in place of the module's ``random``: every draw is kept as
(low, high, value), in order.  The samples are assembled as load_data_sceneflow assembles them
(stereo.py:45-53: planes 0-5 standardised, 6 the left disparity, 7 the right).

Writes tests/golden/train_transform.npz: per case the uint8 inputs, the two disparities, the
three outputs, the draws and the arguments.  Data only; needs the reference's tree.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_transform.py REFERENCE_ROOT
"""
from __future__ import annotations

import importlib.util
import os
import random
import sys

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

# (h, w, crop_h, crop_w, use_left, left_right, shift, seed); the seeds were chosen so that the
# two (F, T, 0) cases see both coins and the shifted cases a shift_x of either sign that
# survives (cases 3, 6, 10) and one that the reset rule zeroes (case 8)
CASES = [
    (10, 14, 6, 8, 1, 0, 0, 1), (10, 14, 6, 8, 0, 1, 0, 2), (10, 14, 6, 8, 0, 0, 0, 3), (10, 14, 6, 8, 1, 0, 3, 4),
    (5, 7, 6, 8, 1, 0, 0, 6), (5, 7, 6, 8, 0, 1, 0, 5), (5, 7, 6, 8, 1, 0, 2, 7),
    (10, 7, 6, 8, 1, 0, 0, 8), (10, 7, 6, 8, 1, 0, 2, 9),
    (6, 8, 6, 8, 1, 0, 0, 10), (6, 8, 6, 8, 1, 0, 2, 14),
    (6, 14, 6, 8, 1, 0, 0, 12),
]


class RecordingRandom:
    """Stands in for the ``random`` module inside common.py: same generator, draws recorded."""

    def __init__(self):
        self.draws = []

    def randint(self, a, b):
        v = random.randint(a, b)
        self.draws.append((a, b, v))
        return v


def case_inputs(i, h, w):
    rng = np.random.default_rng(20261019 + i)
    left = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    # disparities either side of 0 and of a maxdisp of 48, so that a shift moves pixels
    # across both bounds of the validity mask
    dl = rng.uniform(-3, 56, (h, w)).astype(np.float32)
    dr = rng.uniform(-3, 56, (h, w)).astype(np.float32)
    dl[0, 0], dr[0, 0] = 0.0, 0.001
    return left, right, dl, dr


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    spec = importlib.util.spec_from_file_location(
        "ref_common", os.path.join(ref, "dataloaders", "datasets", "common.py"))
    common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(common)
    arrays = {"cases": np.array(CASES, dtype=np.int64)}
    for i, (h, w, ch, cw, ul, lr, shift, seed) in enumerate(CASES):
        left, right, dl, dr = case_inputs(i, h, w)
        temp = np.zeros([8, h, w], "float32")
        common.set_rgb_layers(temp, left, right)
        temp[6, :, :] = dl
        temp[7, :, :] = dr
        rec = RecordingRandom()
        common.random = rec
        random.seed(seed)
        try:
            ol, orr, ot = common.train_transform(temp, ch, cw, use_left=bool(ul), left_right=bool(lr), shift=shift)
        finally:
            common.random = random
        k = f"{i}/"
        arrays[k + "left_u8"], arrays[k + "right_u8"] = left, right
        arrays[k + "disp_left"], arrays[k + "disp_right"] = dl, dr
        arrays[k + "out_left"] = np.ascontiguousarray(ol, dtype=np.float32)
        arrays[k + "out_right"] = np.ascontiguousarray(orr, dtype=np.float32)
        arrays[k + "out_target"] = np.ascontiguousarray(ot)
        assert ot.dtype == np.float32 and ol.shape == (3, ch, cw) and ot.shape == (1, ch, cw)
        arrays[k + "draws"] = np.array(rec.draws, dtype=np.int64).reshape(-1, 3)
        print(i, (h, w, ch, cw), "use_left", ul, "left_right", lr, "shift", shift, "seed", seed, "draws", rec.draws)
    path = os.path.join(GOLD, "train_transform.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
