"""Pin the CPU oracle (oracle/torch_ref.py) against golden vectors produced by
running the reference itself (tools/gen_golden.py; architectures other than the shipped
one: tools/gen_golden_arch.py).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import torch_ref as ref
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from leastereo_amd.weights import state_dict_sha256, synthetic_state_dict
from tests.golden_util import GOLD, arch, golden, meta, normal, state_dict

CASES = meta()["cases"]


def _cases(prefix):
    return sorted(k.split("/", 1)[1] for k in CASES if k.startswith(prefix + "/"))


def test_weight_recipe_hash():
    sd = state_dict()
    assert len(sd) == meta()["n_tensors"] == 918


@pytest.mark.parametrize("name", _cases("cost_volume"))
def test_cost_volume_bit_exact(name):
    c = CASES["cost_volume/" + name]
    fl = normal(c["seeds"][0], c["shape"])
    fr = normal(c["seeds"][1], c["shape"])
    out = ref.build_cost_volume(fl, fr, c["maxdisp"]).numpy()
    np.testing.assert_array_equal(out, golden("cost_volume")[name])


@pytest.mark.parametrize("name", _cases("convbr"))
def test_convbr(name):
    c = CASES["convbr/" + name]
    x = normal(c["seed"], c["input"])
    out = ref.conv_br(x, state_dict(), c["module"], bn=c["bn"], relu=c["relu"]).numpy()
    np.testing.assert_allclose(out, golden("convbr")[name], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", _cases("resample"))
def test_resample(name):
    c = CASES["resample/" + name]
    out = ref.resample_ac(normal(c["seed"], c["input"]), c["size"]).numpy()
    np.testing.assert_allclose(out, golden("resample")[name], rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", _cases("disp"))
def test_disp(name):
    c = CASES["disp/" + name]
    x = normal(c["seed"], c["input"]) * c["gain"]
    out = ref.disp_forward(x, c["maxdisp"]).numpy()
    np.testing.assert_allclose(out, golden("disp")[name], rtol=0, atol=1e-5)


def test_scale_dimension_and_levels():
    assert [ref.scale_dimension(n, 0.5) for n in (64, 65, 85)] == [32, 33, 43]
    assert [ref.scale_dimension(n, 2) for n in (32, 33)] == [64, 65]
    lv = ref.cell_levels(ref.network_layer_to_space(arch()["net_arch_mat"]))
    assert [l for l, _ in lv] == [1, 1, 2, 2, 1, 2, 2, 2, 1, 1, 0, 1]
    assert [d for _, d in lv] == [-1, 0, -1, 0, 1, -1, 0, 0, 1, 0, 1, -1]


@pytest.mark.parametrize("name", _cases("e2e"))
def test_e2e(name):
    c = CASES["e2e/" + name]
    shape = (c["batch"], 3, c["height"], c["width"])
    left, right = normal(c["seeds"][0], shape), normal(c["seeds"][1], shape)
    g = golden("e2e")
    with torch.no_grad():
        st = ref.leastereo_forward(state_dict(), left, right, c["maxdisp"], arch(), return_stages=True)
    if name + "/fea_l" in g:
        np.testing.assert_allclose(st["fea_l"].numpy(), g[name + "/fea_l"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(st["matching"].numpy(), g[name + "/matching"], rtol=1e-4, atol=1e-3)
    d32 = st["disp"]
    assert ref.epe(d32, torch.from_numpy(g[name + "/disp32"])) < 1e-4
    assert ref.epe(d32, torch.from_numpy(g[name + "/disp64"])) < 1e-4


with open(os.path.join(GOLD, "arch_variants.json")) as _f:
    ARCH_CASES = json.load(_f)["cases"]
ARCH_KEYS = ("net_arch_fea", "cell_arch_fea", "net_arch_mat", "cell_arch_mat")


@pytest.mark.parametrize("name", sorted(ARCH_CASES))
def test_arch_variants(tmp_path, name):
    """Genotypes and level paths other than the shipped ones: the oracle in float32 against the
    reference's float32 feature map and matching cost, at test_e2e's tolerances.  The weights are
    the recipe without the calibrated BN file, on the shapes of the model built from the case's
    four arrays (held to the hash of what the reference's own model was loaded with)."""
    c = ARCH_CASES[name]
    a = {k: np.array(c[k]) for k in ARCH_KEYS}
    args = LEAStereoArgs(maxdisp=c["maxdisp"])
    for k in ARCH_KEYS:
        setattr(args, k, str(tmp_path / (k + ".npy")))
        np.save(getattr(args, k), a[k])
    m = LEAStereo(default_arch_args(args), "cpu")
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    assert len(sd) == c["n_tensors"] and state_dict_sha256(sd) == c["state_dict_sha256"]
    shape = (c["batch"], 3, c["height"], c["width"])
    left, right = normal(c["seeds"][0], shape), normal(c["seeds"][1], shape)
    g = golden("arch_variants")
    with torch.no_grad():
        st = ref.leastereo_forward(sd, left, right, c["maxdisp"], a, return_stages=True)
    assert list(st["fea_l"].shape) == c["shapes"]["fea_l"] and list(st["matching"].shape) == c["shapes"]["matching"]
    np.testing.assert_allclose(st["fea_l"].numpy(), g[name + "/fea_l"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(st["matching"].numpy(), g[name + "/matching"], rtol=1e-4, atol=1e-3)
