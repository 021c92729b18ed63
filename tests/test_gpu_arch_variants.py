"""The cell-graph executors on architectures other than the shipped one, on the device.

The executors plan their launches from whatever genotype and level path the model is built with,
and carry many routes tuned for the shipped SceneFlow architecture (the s1 sibling group and its
48-channel split, the pair steps, `share` and the two-head `fanout` launch, the factored stem0
with windowed maps, the "write one level down in the epilogue" routes of the stems, conv1 and
cell 10).  Which of them run is decided by genotype- and path-dependent predicates; here the
genotypes and paths of tests/arch_variants.py (a skip term inside a cell, three-term steps, no s1
group, a state made of skips only, one op per step; paths ending at every level, cell 10 at L1,
`share` on other cells) run through every executor against oracle/torch_ref.py in float64 on the
same inputs and weights -- itself pinned to the reference on these architectures
(tests/test_oracle_golden.py::test_arch_variants).

Every case runs under kernels.KernelProbe and asserts the launches of the device routes, present
and absent, as worked out from the plan (tests/arch_variants.PLANNED, by the level path alone) and
the library's name / *_supported queries -- never from a run's own output: a case that falls back
to the generic launches fails.  The f32 cases run again with the routes switched off.

Weights: the synthetic recipe without the calibrated BN file (kaiming convs, random BN affine,
identity running statistics; the BN file's tensors have the shipped architecture's shapes).  With
them the reference's own float32 disparity is 0.06-0.12 px off its float64 one, so the compared
quantities are the feature maps and the matching cost, as in tests/test_gpu_heads.py.

Bars (tests/test_gpu_heads.py's): f32 and f32_direct max |d| <= 1e-4 * max |ref| + 1e-6; bf16
mean |d| <= 2e-2 * mean |ref|.  Each case prints its error, the bar and E32, the oracle's own
float32-vs-float64 error on the case (pytest -s).  Measured on an MI355X: every f32 and f32_direct
error is 0.47-1.7 x its E32 and 0.01-0.12 of its bar, so no case needed a bar of its own; the
bf16 errors are 0.24-0.99 of theirs (the closest: the feature net of `skip_only_state` on the
shipped path, mean |d| 8.57e-2 against 8.70e-2; the matching net of `s1_last` x `end3`, 24.9
against 29.0).  One conv read as a skip by the oracle: 1.7e4 (matching) and 7.5e3 (feature) x
the bar."""
import contextlib
from collections import Counter

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, executor, kernels
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from leastereo_amd.weights import synthetic_state_dict
from oracle import torch_ref as ref
from tests.arch_variants import (CELL10_DOWN_GENOTYPES, CELL10_DOWN_PATHS, FEATURE_GENOTYPES, MATCHING_GENOTYPES,
                                 MATCHING_PATHS, PLANNED, STEP_BRANCHES, arch_with, random_genotype)
from tests.golden_util import arch, normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAXDISP = 48
ARCH_KEYS = ("net_arch_fea", "cell_arch_fea", "net_arch_mat", "cell_arch_mat")

# (matching genotype, level path, batch); random feature maps [B, 32, 32, 64]: the cost volume
# (16, 32, 64), the smallest at which the stems' and conv1's down-sampling epilogues and the
# factored stem0 are taken
SMALL = (32, 64)
MATCHING_CASES = [
    ("with_skip", "shipped", 1),
    ("seven_convs", "shipped", 1),
    ("seven_convs", "end0", 2),
    ("no_s1_group", "zigzag", 1),
    ("no_s1_group", "up_then_down_L1", 1),
    ("skip_only_state", "start0_end2", 1),
    ("s1_last", "end3", 1),
    ("shipped", "zigzag", 1),
]
# cell 10's down route needs the Winograd engine on its 8 -> 8 ops: (16, 96, 96) x 2 (the 32-wide
# depth-paired tile, <8>) and (16, 96, 192) (the 64-wide one, <16>); the last two must decline (a
# skip term left to add; cell 10 at L1, whose 16-channel ops have no depth-paired tile)
CELL10_CASES = [  # (genotype, path, batch, feature map size, the route is taken)
    ("seven_convs", "shipped", 2, (96, 96), True),
    ("no_s1_group", "zigzag", 1, (96, 192), True),
    ("s1_last", "shipped", 1, (96, 192), True),
    ("with_skip", "shipped", 1, (96, 192), False),
    ("shipped", "up_then_down_L1", 1, (96, 192), False),
]
_CASE_KEYS = [c + (SMALL,) for c in MATCHING_CASES] + [c[:4] for c in CELL10_CASES]
FEATURE_CASES = [  # (feature genotype, level path)
    ("group_covers_pair", "shipped"),
    ("skips_and_group", 2),
    ("skip_only_state", "shipped"),
    ("three_terms", 3),
    ("one_branch", 1),
]


# ------------------------------------------------------------------------------- models
_SD = {}


def _model(tmp, a, precision):
    """LEAStereo of architecture ``a`` (the four arrays) at ``precision`` with the synthetic
    weights, as tests/test_gpu_heads.py::_model; returns (model, state dict)."""
    args = LEAStereoArgs(maxdisp=MAXDISP)
    for k in ARCH_KEYS:
        setattr(args, k, str(tmp / (k + ".npy")))
        np.save(getattr(args, k), np.asarray(a[k]))
    m = LEAStereo(default_arch_args(args), DEV, precision=precision)
    key = tuple(np.asarray(a[k]).tobytes() for k in ARCH_KEYS)
    if key not in _SD:
        _SD[key] = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    m.load_state_dict(_SD[key], strict=True)
    return m.to(DEV).eval(), _SD[key]


def _f64(sd, dev):
    return {k: (v.double() if v.is_floating_point() else v).to(dev) for k, v in sd.items()}


@contextlib.contextmanager
def _switches(m, **kw):
    """MatchingExecutor's class switches set for the block; the plan is made when the executor is
    built, so it is dropped on the way in and out."""
    cls = executor.MatchingExecutor
    old = {k: getattr(cls, k) for k in kw}
    for k, v in kw.items():
        setattr(cls, k, v)
    m.matching.invalidate()
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(cls, k, v)
        m.matching.invalidate()


def _bar(got, want, precision):
    """(error, bar, scale) of ``got`` against the float64 ``want`` at the precision's bar."""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    if precision == "bf16":
        err, scale = float((got - want).abs().mean()), float(want.abs().mean())
        return err, 2e-2 * scale, scale
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    return err, 1e-4 * scale + 1e-6, scale


# ------------------------------------------------------------------ the matching net's routes
ROUTES = ("conv1x1_heads_kernel<", "conv3d_wino44_down2_kernel", "conv3d_wino44_down2_cat_kernel",
          "conv3d_wino_dp_down2_kernel<", "resample3d_sep_down2_f32", " windowed", "cv_stem_f32_down2_kernel",
          "bf16 pair")


def _levels(a):
    return [lv for lv, _ in ref.cell_levels(ref.network_layer_to_space(a["net_arch_mat"]))]


def _expected_routes(me, a, geno, path, b, vol):
    """The device routes' launches that executor ``me`` must issue on an L0 volume ``vol``, by
    name, from the plan (PLANNED: what the level path alone decides; the genotypes whose cell 10
    is finished by conv launches) and the library's own queries at the shapes -- every volume here
    halves exactly at every level."""
    lib = _lib.load()
    plan, levels = PLANNED[path], _levels(a)
    at = lambda lv: tuple(n >> lv for n in vol)
    f32 = type(me) is executor.MatchingExecutor
    exp = {r: [] for r in ROUTES}
    if f32 and me.FANOUT_1X1:
        exp["conv1x1_heads_kernel<"] = [None] * len(plan["fanout"])
    if f32 and me.WINDOWED_MAPS and kernels.cv_stem_supported(32, vol[0], vol[2], False):
        exp[" windowed"] = [None, None]   # the left and the right maps
    if f32 and me.FUSED_DOWN and plan["cell0_down"]:
        if kernels.cv_stem_supported(32, vol[0], vol[2], False) and lib.lea_cv_stem_down2_supported(32, *vol, _lib.LEA_F32):
            exp["cv_stem_f32_down2_kernel"] = ["cv_stem_f32_down2_kernel"]
        if 0 in plan["share"] and kernels.wino_preferred(b, 32, 32, *vol):
            name = kernels.wino_down2_kernel_name(b, 32, 32, *vol)
            exp["conv3d_wino44_down2_kernel"] = [name] if name is not None else []
    l1 = at(1)  # cells 1 and 4 sit at level 1 on every path: conv1 is 64 + 64 -> 64 there
    if f32 and me.FUSED_DOWN_CELLS and plan["conv1_down"] and kernels.wino_preferred(b, 64, 128, *l1):
        name = kernels.wino_down2_kernel_name(b, 128, 64, *l1, 64)
        exp["conv3d_wino44_down2_cat_kernel"] = [name] if name is not None else []
    c10, s10 = 8 << levels[10], at(levels[10])
    if isinstance(geno, str):
        cell10 = geno in CELL10_DOWN_GENOTYPES and path in CELL10_DOWN_PATHS
        if f32 and me.FUSED_DOWN_CELLS:
            assert me._cell_output_takes_down(10, s10) == cell10
    else:  # a drawn genotype: whatever the predicate says, at a volume where the route cannot be taken
        cell10 = False
        assert not kernels.wino_preferred(b, c10, c10, *s10)
    if (f32 and me.FUSED_DOWN_CELLS and cell10 and kernels.wino_preferred(b, c10, c10, *s10)
            and kernels.wino_dp_down2_kernel_name(b, c10, c10, *s10) is not None
            and kernels.resample_down2_shape_supported(at(levels[9]), s10)):
        # s1's up-sampling writes the level-down copy; each step's finishing launch too, the last
        # state's alone (`only`)
        exp["resample3d_sep_down2_f32"] = ["resample3d_sep_down2_f32"]
        exp["conv3d_wino_dp_down2_kernel<"] = [kernels.wino_dp_down2_kernel_name(b, c10, c10, *s10, only)
                                               for only in (False, False, True)]
    if type(me) is executor.MatchingExecutorBF16:
        # the pair steps: a genotype whose every step sums exactly two conv ops, in every cell
        rows = a["cell_arch_mat"].tolist()
        paired = all([p for br, p in rows if br in step] == [1, 1] for step in STEP_BRANCHES)
        assert sorted(me.pair_steps) == (list(range(12)) if paired else [])
        for i in sorted(me.pair_steps):
            c, v = 8 << levels[i], at(levels[i])
            if lib.lea_conv3d_bf16_pair_supported(b, c, c, *v):
                name = kernels.conv_kernel_name_bf16(b, c, 2 * c, *v, 3, cin2=c, flags=_lib.LEA_PAIR_SUM)
                assert name is not None
                exp["bf16 pair"] += [(name, (b, 2 * c, c) + v + (3,))] * 3
    return exp


def _taken_routes(records):
    """The same table from a probe's records."""
    got = {r: [] for r in ROUTES}
    for r in records:
        if r.name.startswith("conv1x1_heads_kernel<"):
            got["conv1x1_heads_kernel<"].append(None)
        elif r.name.endswith(" windowed"):
            got[" windowed"].append(None)
        elif r.name.startswith("conv3d_wino_dp_down2_kernel<"):
            got["conv3d_wino_dp_down2_kernel<"].append(r.name)
        elif r.name in ROUTES:
            got[r.name].append(r.name)
        elif (r.name.startswith("conv_bf16") and r.shape is not None and r.shape[6] == 3
              and r.shape[1] == 2 * r.shape[2] and r.shape[2] <= 16):
            got["bf16 pair"].append((r.name, tuple(r.shape)))   # two c-channel sources -> c: a pair step
    return got


def _check_plan(me, path):
    """The routes that the level path alone decides, as planned on the device build."""
    plan = PLANNED[path]
    assert {i for i in range(12) if f"cells.{i}.share" in me.p} == plan["share"]
    fanout = plan["fanout"] if me.FANOUT_1X1 else set()
    assert {i for i in range(12) if f"cells.{i}.fanout" in me.p} == fanout


def _run_matching(m, case, geno, path, what=""):
    """One forward of the matching net from the case's feature maps under the probe; the routes
    taken must be the expected ones.  Returns (matching cost, the routes taken)."""
    me = m.matching.executor()
    b, vol = case["fl"].shape[0], (MAXDISP // 3,) + tuple(case["fl"].shape[2:])
    _check_plan(me, path)
    exp = _expected_routes(me, case["a"], geno, path, b, vol)
    with torch.no_grad(), kernels.KernelProbe() as probe:
        got = me.run_features(case["fl"].to(DEV), case["fr"].to(DEV), MAXDISP)
    taken = _taken_routes(probe.records)
    print(f"{geno} x {path} b{b} {vol} {type(me).__name__}{what}: routes "
          + (", ".join(f"{len(v)} x {k.strip()}" for k, v in taken.items() if v) or "none"))
    for r in ROUTES:  # (the depth-paired launches in their order: the `only` form finishes the last state)
        assert taken[r] == exp[r] or (r != "conv3d_wino_dp_down2_kernel<"
                                      and sorted(taken[r], key=str) == sorted(exp[r], key=str)), (r, taken[r], exp[r])
    return got, taken


@pytest.fixture(scope="module")
def matching_case(tmp_path_factory):
    """Per (genotype, path, batch, feature map size): the architecture, seeded feature maps, the
    float64 oracle's matching cost (computed on the device with torch) and E32, the float32
    oracle's distance from it (on the host); computed once for every executor and switch."""
    memo = {}

    def get(geno, path, b, hw, seed=None):
        key = (str(geno), path, b, hw)
        if key not in memo:
            a = arch_with(arch(), mat_geno=geno, mat_path=path)
            g = torch.Generator().manual_seed(7000 + _CASE_KEYS.index(key) if seed is None else seed)
            fl = torch.randn((b, 32) + hw, generator=g)
            fr = torch.randn((b, 32) + hw, generator=g)
            _, sd = _model(tmp_path_factory.mktemp("arch"), a, "f32")
            with torch.no_grad():
                cost = ref.build_cost_volume(fl.double().to(DEV), fr.double().to(DEV), MAXDISP)
                want = ref.matching_forward(_f64(sd, DEV), cost, a["net_arch_mat"], a["cell_arch_mat"]).cpu()
                del cost
                want32 = ref.matching_forward(sd, ref.build_cost_volume(fl, fr, MAXDISP), a["net_arch_mat"],
                                              a["cell_arch_mat"])
            e32 = float((want32.double() - want).abs().max())
            memo[key] = dict(a=a, fl=fl, fr=fr, want=want, e32=e32, sd=sd)
        return memo[key]
    return get


def _report(tag, precision, err, bar, scale, e32):
    print(f"{tag} {precision}: err {err:.3e} bar {bar:.3e} ({'mean' if precision == 'bf16' else 'max'} |ref| "
          f"{scale:.3e}); oracle f32 vs f64 E32 {e32:.3e} max")


@pytest.mark.parametrize("precision", ["f32", "f32_direct", "bf16"])
@pytest.mark.parametrize("geno,path,b", MATCHING_CASES)
def test_matching_variant(tmp_path, matching_case, geno, path, b, precision):
    case = matching_case(geno, path, b, SMALL)
    m, _ = _model(tmp_path, case["a"], precision)
    m.check_shape(3 * SMALL[0], 3 * SMALL[1])
    got, taken = _run_matching(m, case, geno, path)
    err, bar, scale = _bar(got, case["want"], precision)
    _report(f"{geno} x {path} b{b}", precision, err, bar, scale, case["e32"])
    assert err <= bar, (err, bar)
    if precision != "f32":
        return
    # the routes that change no arithmetic off: the same bits; the down-sampling epilogues off
    # (their readers' 1x1 sums associate differently): the same bar
    with _switches(m, FANOUT_1X1=False, WINDOWED_MAPS=False):
        plain, off = _run_matching(m, case, geno, path, " fanout / windowed maps off")
    assert not off["conv1x1_heads_kernel<"] and not off[" windowed"]
    assert torch.equal(plain, got)
    with _switches(m, FUSED_DOWN=False, FUSED_DOWN_CELLS=False):
        plain, off = _run_matching(m, case, geno, path, " down-sampling epilogues off")
    assert not any(off[r] for r in ROUTES if "down2" in r)
    err, bar, scale = _bar(plain, case["want"], precision)
    _report(f"{geno} x {path} b{b} epilogues off", precision, err, bar, scale, case["e32"])
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("geno,path,b,hw,takes", CELL10_CASES)
def test_cell10_down_route(tmp_path, matching_case, geno, path, b, hw, takes):
    """Cell 10's producers write the last cell's level where its genotype and path allow it and
    the depth-paired tile exists, and decline otherwise (f32)."""
    case = matching_case(geno, path, b, hw)
    m, _ = _model(tmp_path, case["a"], "f32")
    got, taken = _run_matching(m, case, geno, path)
    q = 8 if hw[1] == 96 else 16
    assert taken["conv3d_wino_dp_down2_kernel<"] == ([f"conv3d_wino_dp_down2_kernel<{q}, false>"] * 2
                                                    + [f"conv3d_wino_dp_down2_kernel<{q}, true>"]) * int(takes)
    assert len(taken["resample3d_sep_down2_f32"]) == int(takes)
    err, bar, scale = _bar(got, case["want"], "f32")
    _report(f"{geno} x {path} b{b} {hw}", "f32", err, bar, scale, case["e32"])
    assert err <= bar, (err, bar)
    with _switches(m, FANOUT_1X1=False, WINDOWED_MAPS=False):
        plain, _ = _run_matching(m, case, geno, path, " fanout / windowed maps off")
    assert torch.equal(plain, got)
    with _switches(m, FUSED_DOWN=False, FUSED_DOWN_CELLS=False):
        plain, off = _run_matching(m, case, geno, path, " down-sampling epilogues off")
    assert not any(off[r] for r in ROUTES if "down2" in r)
    err, bar, scale = _bar(plain, case["want"], "f32")
    _report(f"{geno} x {path} b{b} {hw} epilogues off", "f32", err, bar, scale, case["e32"])
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("seed", range(10))
def test_matching_drawn_genotype(tmp_path, matching_case, seed, precision):
    """Seeded random genotypes x level paths (the CPU sweep's recipe, tests/test_executor_plan_cpu.py)
    on the device: the bar, and the routes that the level path decides."""
    rng = np.random.default_rng(7300 + seed)
    geno = random_genotype(rng, shuffle=bool(seed % 2))
    path = sorted(MATCHING_PATHS)[int(rng.integers(len(MATCHING_PATHS)))]
    case = matching_case(geno, path, 1, SMALL, seed=7400 + seed)
    m, _ = _model(tmp_path, case["a"], precision)
    got, _ = _run_matching(m, case, geno, path)
    err, bar, scale = _bar(got, case["want"], precision)
    _report(f"{geno} x {path}", precision, err, bar, scale, case["e32"])
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------- the feature net
def _expected_feature_convs(fe, a, b, h, w):
    """The FLOPs of every 3x3 launch of a feature-net forward, counted, from the plan: stem2
    (32 -> 32 at the full size; the head's convs are 1x1), and per cell the s1 sibling group (one
    launch of n * c couts), the s0 pair (one of 2 c) and a launch per remaining conv op."""
    levels = [lv for lv, _ in ref.cell_levels(ref.network_layer_to_space(a["net_arch_fea"]))]
    flops = lambda cout, cin, lv: 2.0 * b * (h >> lv) * (w >> lv) * cout * cin * 9
    exp = Counter({flops(32, 32, 0): 1})
    for i, cell in enumerate(fe.m.cells):
        c, lv = cell.c_out, levels[i]
        assert c == 8 << lv
        ops = {(k, op) for k, terms in enumerate(cell.plan) for op, _ in terms if cell.op_kinds[op] == "conv"}
        group, pair = fe.s1_group.get(i, []), fe.s0_pair.get(i)
        if group:
            exp[flops(len(group) * c, c, lv)] += 1
            ops -= set(group)
        if pair:
            exp[flops(2 * c, c, lv)] += 1
            ops -= set(pair)
        exp[flops(c, c, lv)] += len(ops)
    return +exp


@pytest.fixture(scope="module")
def feature_case(tmp_path_factory):
    memo = {}

    def get(geno, path):
        key = (geno, path)
        if key not in memo:
            a = arch_with(arch(), fea_geno=geno, fea_path=path)
            x = normal(7600 + FEATURE_CASES.index(key), (2, 3, 96, 192))
            _, sd = _model(tmp_path_factory.mktemp("arch"), a, "f32")
            with torch.no_grad():
                want = ref.feature_forward(_f64(sd, DEV), x.double().to(DEV), a["net_arch_fea"], a["cell_arch_fea"]).cpu()
                want32 = ref.feature_forward(sd, x, a["net_arch_fea"], a["cell_arch_fea"])
            memo[key] = dict(a=a, x=x, want=want, e32=float((want32.double() - want).abs().max()), sd=sd)
        return memo[key]
    return get


def _run_feature(m, case, precision):
    fe = m.feature.executor()
    x = case["x"]
    exp = _expected_feature_convs(fe, case["a"], x.shape[0], 32, 64)
    with torch.no_grad(), kernels.KernelProbe() as probe:
        got = m.feature(x.to(DEV))
    names = [r.name for r in probe.records]
    assert names.count("feature_stem_kernel") == 1   # stems 0 and 1 fused, whatever the cells are
    convs = Counter(r.flops for r in probe.records if r.flops in exp)
    assert convs == exp, (convs, exp)
    if precision == "bf16":
        assert got.dtype == torch.bfloat16 and got.dim() == 6
        got = kernels.from_c8(got)[:, :, 0]
    return got, fe


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("geno,path", FEATURE_CASES)
def test_feature_variant(tmp_path, feature_case, geno, path, precision):
    case = feature_case(geno, path)
    m, _ = _model(tmp_path, case["a"], precision)
    got, fe = _run_feature(m, case, precision)
    pairs, groups = sorted(fe.s0_pair), {i: len(g) for i, g in fe.s1_group.items()}
    print(f"feature {geno} x {path} {precision}: s0 pair in cells {pairs}, s1 groups {groups}")
    # a group that covers a step of the pair keeps the pair off; the pair is the f32 few-channel
    # tile's (cells of 8 and 16 channels)
    if precision == "bf16" or geno in ("group_covers_pair", "skips_and_group", "three_terms", "one_branch"):
        assert not pairs
    else:
        assert pairs == [i for i, c in enumerate(fe.m.cells) if c.c_out <= 16] and pairs
    assert bool(groups) == (geno in ("group_covers_pair", "skips_and_group", "one_branch"))
    err, bar, scale = _bar(got, case["want"], precision)
    _report(f"feature {geno} x {path}", precision, err, bar, scale, case["e32"])
    assert err <= bar, (err, bar)


# -------------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_model_is_its_executors_chained(tmp_path, precision):
    """model(left, right) is, bit for bit, Disp of run_features on the feature executor's own
    output -- at bf16 the c8 hand-off from FeatureExecutorBF16 to MatchingExecutorBF16 (the same
    bits as handing over its f32 copy) -- on a non-shipped architecture; and the matching cost
    meets the bar against the oracle on those feature maps."""
    a = arch_with(arch(), "skips_and_group", 2, "no_s1_group", "zigzag")
    m, sd = _model(tmp_path, a, precision)
    left, right = normal(7801, (1, 3, 96, 192)).to(DEV), normal(7802, (1, 3, 96, 192)).to(DEV)
    with torch.no_grad():
        disp = m(left, right)
        f = m.feature(left, right)
        cost = m.matching.executor().run_features(f[:1], f[1:], MAXDISP)
        assert torch.equal(disp, m.disp(cost, fast_exp=precision == "bf16"))
        f32 = f
        if precision == "bf16":
            assert f.dtype == torch.bfloat16 and f.dim() == 6
            f32 = kernels.from_c8(f)[:, :, 0]
            assert torch.equal(cost, m.matching.executor().run_features(f32[:1], f32[1:], MAXDISP))
        vol = ref.build_cost_volume(f32[:1].double(), f32[1:].double(), MAXDISP)
        want = ref.matching_forward(_f64(sd, DEV), vol, a["net_arch_mat"], a["cell_arch_mat"])
    err, bar, scale = _bar(cost, want, precision)
    print(f"chained {precision}: matching cost err {err:.3e} bar {bar:.3e}")
    assert disp.shape == (1, 96, 192) and bool(torch.isfinite(disp).all())
    assert err <= bar, (err, bar)


# ----------------------------------------------------------------------------- sensitivity
def _flipped(rows, row):
    """The genotype with ``row``'s conv made a skip (the oracle then leaves that op's weights out)."""
    rows = [list(r) for r in rows]
    assert rows[row][1] == 1
    rows[row][1] = 0
    return np.array(rows)


def test_matching_check_sees_one_wrong_primitive(tmp_path, matching_case):
    """The comparison can fail: against the oracle of a genotype that differs in one row's
    primitive (a conv read as a skip) the error is more than ten times the bar."""
    geno, path = "seven_convs", "shipped"
    case = matching_case(geno, path, 1, SMALL)
    m, sd = _model(tmp_path, case["a"], "f32")
    got, _ = _run_matching(m, case, geno, path)
    with torch.no_grad():
        cost = ref.build_cost_volume(case["fl"].double().to(DEV), case["fr"].double().to(DEV), MAXDISP)
        wrong = ref.matching_forward(_f64(sd, DEV), cost, case["a"]["net_arch_mat"],
                                     _flipped(MATCHING_GENOTYPES[geno], 4))
    err, bar, _ = _bar(got, wrong, "f32")
    print(f"one primitive off: err {err:.3e} bar {bar:.3e}")
    assert err > 10 * bar


def test_feature_check_sees_one_wrong_primitive(tmp_path, feature_case):
    geno, path = "group_covers_pair", "shipped"
    case = feature_case(geno, path)
    m, sd = _model(tmp_path, case["a"], "f32")
    got, _ = _run_feature(m, case, "f32")
    with torch.no_grad():
        wrong = ref.feature_forward(_f64(sd, DEV), case["x"].double().to(DEV), case["a"]["net_arch_fea"],
                                    _flipped(FEATURE_GENOTYPES[geno], 3))
    err, bar, _ = _bar(got, wrong, "f32")
    print(f"one primitive off: err {err:.3e} bar {bar:.3e}")
    assert err > 10 * bar
