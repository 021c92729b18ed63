"""Golden vectors of the REFERENCE on architectures other than the shipped one: five
(feature genotype, feature path, matching genotype, matching path) combinations that together
cover every variant of tests/arch_variants.py.  Per combination the reference model (built from
the four arrays, retrain/LEAStereo.py:12-27) takes the synthetic weights without the calibrated BN
file (synthetic_state_dict(shapes, bn_file=None): the only recipe that exists for other
architectures) and seeded images at 48 x 96 with maxdisp 48 -- a cost volume of (16, 16, 32), the
smallest whose level 3 comes back up through scale_dimension -- and its float32 left feature map
and matching cost are stored.  (Disparity is not: with identity BN statistics the reference's own
float32 disparity differs from its float64 one by ~0.1 px.)

Writes tests/golden/arch_variants.npz and arch_variants.json (the four arrays, seeds and shapes of
each case; tests/test_oracle_golden.py reads the cases from there).

Runs only in the build container (it imports the reference, read-only, with bytecode writing
disabled); only numbers are written.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_arch.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from leastereo_amd.weights import seeded_normal, state_dict_sha256, synthetic_state_dict  # noqa: E402
from tests.arch_variants import arch_with  # noqa: E402
from tests.golden_util import GOLD, arch, save_golden  # noqa: E402
from tools.gen_golden import REF  # noqa: E402

HEIGHT, WIDTH, MAXDISP = 48, 96, 48
# (feature genotype, feature path, matching genotype, matching path)
COMBINATIONS = {
    "a": ("group_covers_pair", 1, "with_skip", "end0"),
    "b": ("skips_and_group", 2, "seven_convs", "start0_end2"),
    "c": ("skip_only_state", 3, "no_s1_group", "end3"),
    "d": ("three_terms", "shipped", "skip_only_state", "up_then_down_L1"),
    "e": ("one_branch", 1, "s1_last", "zigzag"),
}
KEYS = ("net_arch_fea", "cell_arch_fea", "net_arch_mat", "cell_arch_mat")


def ref_model(a, maxdisp, tmp):
    sys.path.insert(0, REF)
    from config_utils.leastereo_args import LEAStereoArgs  # reference: config_utils/leastereo_args.py:16
    from retrain.LEAStereo import LEAStereo  # reference: retrain/LEAStereo.py:12
    paths = {}
    for k in KEYS:
        paths[k] = os.path.join(tmp, k + ".npy")
        np.save(paths[k], np.asarray(a[k]))
    args = LEAStereoArgs(**paths)
    args.maxdisp = maxdisp
    args.cuda = False
    return LEAStereo(args, "cpu")


def main():
    arrays, cases = {}, {}
    for n, (name, combo) in enumerate(COMBINATIONS.items()):
        a = arch_with(arch(), *combo)
        with tempfile.TemporaryDirectory() as tmp:
            model = ref_model(a, MAXDISP, tmp)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd = synthetic_state_dict(shapes, bn_file=None)
        model.load_state_dict(sd, strict=True)
        model.eval()
        seeds = [1101 + 2 * n, 1102 + 2 * n]
        shape = (1, 3, HEIGHT, WIDTH)
        left, right = (torch.from_numpy(seeded_normal(s, shape)) for s in seeds)
        got = {}
        model.disp.register_forward_hook(lambda mod, inp, out: got.setdefault("mat", inp[0].detach().clone()))
        with torch.no_grad():
            fea_l = model.feature(left)
            model(left, right)
        arrays[name + "/fea_l"] = fea_l.numpy().astype(np.float32)
        arrays[name + "/matching"] = got["mat"].numpy().astype(np.float32)
        cases[name] = {"combination": [str(c) for c in combo], "seeds": seeds, "batch": 1, "height": HEIGHT,
                       "width": WIDTH, "maxdisp": MAXDISP,
                       "shapes": {k: list(arrays[name + "/" + k].shape) for k in ("fea_l", "matching")},
                       "n_tensors": len(sd), "state_dict_sha256": state_dict_sha256(sd),
                       **{k: np.asarray(a[k]).tolist() for k in KEYS}}
        print(name, combo, {k: v.shape for k, v in arrays.items() if k.startswith(name + "/")})
    paths = save_golden("arch_variants", arrays)
    with open(os.path.join(GOLD, "arch_variants.json"), "w") as f:
        json.dump({"weights": "synthetic_state_dict(shapes, bn_file=None)", "cases": cases}, f, indent=1, sort_keys=True)
    print("wrote", paths, [os.path.getsize(p) for p in paths])


if __name__ == "__main__":
    main()
