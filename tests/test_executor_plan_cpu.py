"""The cell-graph executors' launch plans, checked on the CPU.

``FeatureExecutor`` (new_model_2d.py:140-165) turns a searched cell into a few fused
launches: the s1 sibling group (one conv writing consecutive cat slots), the s0 pair
(two ops on s0 in one launch writing two slots, lea_conv2d_bnrelu_pair), skip terms as
epilogue residuals and the remaining ops accumulating into their slots.  Which launch
writes a slot first and which accumulate depends on the genotype, so a plan that is
right for the shipped genotype can be wrong for another (a genotype whose
s1 group covers a step of the s0 pair).

These tests replace the library's launches by plain torch ops with the same contract
(tests/executor_stands.py: packed weights = the raw weights; ``out``/``accumulate``/``residual``
semantics of kernels.py) and run the executor in float64 on CPU against the oracle
(oracle/torch_ref.feature_forward, itself pinned to the reference's fixtures): the
executor's graph logic is then the only thing under test.  The HIP arithmetic is
covered by the -m gpu tests.
"""
import numpy as np
import pytest
import torch

from leastereo_amd import executor as ex
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from leastereo_amd.weights import synthetic_state_dict
from oracle import torch_ref as ref
from tests.arch_variants import FEATURE_PATHS, MATCHING_PATHS, PLANNED, arch_with, random_genotype
from tests.executor_stands import Stand
from tests.golden_util import arch, normal


@pytest.fixture
def fake(monkeypatch):
    fk = Stand().install(monkeypatch)
    # the stems as two convs (the fused stem kernel has no stand-in here)
    monkeypatch.setattr(ex.FeatureExecutor, "FUSED_STEM", False)
    return fk


# The shipped genotype, and ones whose s1 sibling group overlaps the steps of the s0 pair
# (rows: (state index, primitive), genotypes_2d.py; primitive 1 = 3x3 conv, 0 = skip)
GENOTYPES = {
    "shipped": None,
    # s0 convs at steps 0 and 2 (a pair), s1 convs at steps 0 and 1 (a group covering step 0)
    "group_covers_pair": [[0, 1], [1, 1], [3, 1], [4, 1], [5, 1], [8, 1]],
    # s1 convs at steps 0, 1, 2 (a group covering both pair steps)
    "group_covers_both": [[0, 1], [1, 1], [3, 1], [2, 1], [5, 1], [6, 1]],
    # s1 group at steps 1, 2 beside an s0 pair at steps 0 and 2, skip terms mixed in
    "skips_and_group": [[0, 1], [1, 0], [3, 1], [4, 1], [5, 1], [6, 1]],
}


@pytest.mark.parametrize("pair_s0", [True, False])
@pytest.mark.parametrize("geno", sorted(GENOTYPES))
def test_feature_executor_plan_matches_oracle(tmp_path, fake, monkeypatch, geno, pair_s0):
    monkeypatch.setattr(ex.FeatureExecutor, "PAIR_S0", pair_s0)
    args = LEAStereoArgs(maxdisp=48)
    a = arch()
    if GENOTYPES[geno] is not None:
        a["cell_arch_fea"] = np.array(GENOTYPES[geno])
        args.cell_arch_fea = str(tmp_path / "fea_geno.npy")
        np.save(args.cell_arch_fea, a["cell_arch_fea"])
    args = default_arch_args(args)
    m = LEAStereo(args, "cpu")
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    m.load_state_dict(sd, strict=True)
    m = m.double().eval()
    fe = ex.FeatureExecutor(m.feature)
    if geno == "shipped" and pair_s0:
        assert fe.s0_pair, "the shipped genotype's cells run their s0 pair as one launch"
    for i, pair in fe.s0_pair.items():  # a pair never shares a step with the s1 group
        assert not ({k for k, _ in fe.s1_group.get(i, [])} & {k for k, _ in pair})
    x = normal(901, (2, 3, 48, 96)).double()
    with torch.no_grad():
        got = fe.run(x)
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        want = ref.feature_forward(sd64, x, a["net_arch_fea"], a["cell_arch_fea"])
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    # folded BN is f32 by design (model.ConvBR.folded_bn): ~1e-7 relative per layer; a plan
    # error (a dropped or doubled term) is O(1)
    assert err <= 1e-5 * float(want.abs().max()), err


# The matching net's cells (skip_model_3d.py:41-75): the shipped genotype (every step two conv
# terms: LEA_PAIR_SUM launches when PAIR_STEPS) and one with a skip term (that cell keeps the
# s1 group + accumulating launches)
MATCHING_GENOTYPES = {"shipped": None, "with_skip": [[1, 1], [0, 1], [3, 1], [4, 0], [8, 1], [6, 1]]}


@pytest.mark.parametrize("pair_steps", [True, False])
@pytest.mark.parametrize("split48", [True, False])
@pytest.mark.parametrize("geno", sorted(MATCHING_GENOTYPES))
def test_matching_executor_plan_matches_oracle(tmp_path, fake, monkeypatch, geno, split48, pair_steps):
    monkeypatch.setattr(ex.MatchingExecutor, "PAIR_STEPS", pair_steps)
    monkeypatch.setattr(ex.MatchingExecutor, "SPLIT_S1_GROUP48", split48)
    monkeypatch.setattr(ex, "CV_STEM", False)
    args = LEAStereoArgs(maxdisp=48)
    a = arch()
    if MATCHING_GENOTYPES[geno] is not None:
        a["cell_arch_mat"] = np.array(MATCHING_GENOTYPES[geno])
        args.cell_arch_mat = str(tmp_path / "mat_geno.npy")
        np.save(args.cell_arch_mat, a["cell_arch_mat"])
    args = default_arch_args(args)
    m = LEAStereo(args, "cpu")
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    m.load_state_dict(sd, strict=True)
    m = m.double().eval()
    me = ex.MatchingExecutor(m.matching)
    if pair_steps and geno == "shipped":
        assert len(me.pair_steps) == len(m.matching.cells), "every shipped cell runs as pair launches"
    if geno == "with_skip":
        assert 0 not in me.pair_steps  # every cell has the skip term at step 1
    x = normal(903, (1, 64, 16, 32, 64)).double()  # the e2e case's cost volume shape (96x192 D48)
    with torch.no_grad():
        got = me.run(x)
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        want = ref.matching_forward(sd64, x, a["net_arch_mat"], a["cell_arch_mat"])
    pairs = [e for e in fake.log if e[0] == "wino" and e[3]]
    assert bool(pairs) == (pair_steps and geno == "shipped")
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), err


# ---- a seeded sweep of random genotypes x level paths (tests/arch_variants.random_genotype: each
# step 1-3 of its branches, a random primitive per row; the row order within a step shuffled for
# every other draw, as the shipped file's is), the route switches drawn with them
def _cpu_model(tmp_path, a):
    args = LEAStereoArgs(maxdisp=48)
    for k in ("net_arch_fea", "cell_arch_fea", "net_arch_mat", "cell_arch_mat"):
        setattr(args, k, str(tmp_path / (k + ".npy")))
        np.save(getattr(args, k), a[k])
    m = LEAStereo(default_arch_args(args), "cpu")
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    m.load_state_dict(sd, strict=True)
    return m.double().eval(), {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _draw(seed, paths):
    rng = np.random.default_rng(seed)
    geno = random_genotype(rng, shuffle=bool(seed % 2))
    path = sorted(paths, key=str)[int(rng.integers(len(paths)))]
    return rng, geno, path


@pytest.mark.parametrize("seed", range(30))
def test_feature_executor_random_genotype_matches_oracle(tmp_path, fake, monkeypatch, seed):
    rng, geno, path = _draw(4100 + seed, FEATURE_PATHS)
    monkeypatch.setattr(ex.FeatureExecutor, "PAIR_S0", bool(rng.integers(2)))
    a = arch_with(arch(), fea_geno=geno, fea_path=path)
    m, sd64 = _cpu_model(tmp_path, a)
    fe = ex.FeatureExecutor(m.feature)
    for i, pair in fe.s0_pair.items():
        assert not ({k for k, _ in fe.s1_group.get(i, [])} & {k for k, _ in pair})
    x = normal(4200 + seed, (2, 3, 48, 96)).double()
    with torch.no_grad():
        got = fe.run(x)
        want = ref.feature_forward(sd64, x, a["net_arch_fea"], a["cell_arch_fea"])
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), (geno, path, err)


@pytest.mark.parametrize("seed", range(30))
def test_matching_executor_random_genotype_matches_oracle(tmp_path, fake, monkeypatch, seed):
    rng, geno, path = _draw(4300 + seed, MATCHING_PATHS)
    monkeypatch.setattr(ex.MatchingExecutor, "PAIR_STEPS", bool(rng.integers(2)))
    monkeypatch.setattr(ex.MatchingExecutor, "SPLIT_S1_GROUP48", bool(rng.integers(2)))
    monkeypatch.setattr(ex, "CV_STEM", False)
    a = arch_with(arch(), mat_geno=geno, mat_path=path)
    m, sd64 = _cpu_model(tmp_path, a)
    me = ex.MatchingExecutor(m.matching)
    # the routes that depend on the level path alone
    plan = PLANNED[path]
    assert {i for i in range(12) if f"cells.{i}.share" in me.p} == plan["share"]
    assert {i for i in range(12) if f"cells.{i}.fanout" in me.p} == plan["fanout"]
    assert me._conv1_takes_down((8, 16, 32)) == plan["conv1_down"]
    assert me._cell0_takes_down((16, 32, 64)) == plan["cell0_down"]
    x = normal(4400 + seed, (1, 64, 16, 32, 64)).double()
    with torch.no_grad():
        got = me.run(x)
        want = ref.matching_forward(sd64, x, a["net_arch_mat"], a["cell_arch_mat"])
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), (geno, path, err)
