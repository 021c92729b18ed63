"""What each executor holds after it is built, checked on the CPU: the entries of ``p``, the plans
(``s1_group``, ``s1_split``, ``s0_pair``, ``pair_steps``), and for every entry the weight it launches
with -- ``wino`` where it is set, else ``packed`` -- against an expectation built here from the
modules' own weights.  The six ``kernels.pack_*`` functions are counting stand-ins that return a
copy of their argument, so a packed weight is the stacked source weight itself and a stacking
mistake (order, axis, a missing zero row) is a plain mismatch.

The shipped net, default switches, ``CV_STEM`` off (the weight split of the factored stem is a
device kernel).  The entry counts and plans below were recorded from the tree before the executors
planned their entries in one place and packed them once; the contents tests pass on that tree
unedited.  The pack-call tests at the end describe the tree that packs once, in the format that
runs."""
import collections

import pytest
import torch

from leastereo_amd import executor as ex
from leastereo_amd import kernels
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from leastereo_amd.weights import synthetic_state_dict

PACKERS = ("pack_conv_weight", "pack_conv2d_weight", "pack_conv2d_weight_windowed", "pack_conv_weight_wino",
           "pack_conv_weight_bf16", "pack_conv2d_weight_bf16")
F32_PACKERS = PACKERS[:4]

# the shipped genotypes' plans, as recorded: the matching cells' ops on s1 (one per step), their
# steps as (op, state) pairs, and the feature cells' two conv ops on s0
GROUP = [(0, 1), (1, 2), (2, 4)]
STEPS = [[(0, 0), (1, 1)], [(2, 1), (3, 2)], [(4, 1), (5, 3)]]
S0_PAIR = [(0, 0), (2, 4)]
SPLIT = {0, 1, 4, 8, 9, 11}          # the 16-channel matching cells
SHARE = [0, 2, 5, 8]                 # matching cells that down-sample before a same-level cell
FANOUT = [3, 4, 6, 7, 9, 10]

# executor -> (net, entries, {stacked kind: count}, s1_group cells, s1_split, s0_pair cells, pair_steps cells)
HOLDS = {
    "MatchingExecutor": ("matching", 133, {"s1_group_head": 6, "s1_group": 12, "share": 4, "fanout": 6},
                         range(12), SPLIT, (), ()),
    "MatchingExecutorDirect": ("matching", 121, {"s1_group": 12, "share": 4}, range(12), set(), (), ()),
    "MatchingExecutorBF16": ("matching", 157, {"s1_group": 12, "share": 4, "pair0": 12, "pair1": 12, "pair2": 12},
                             range(12), set(), (), range(12)),
    "FeatureExecutor": ("feature", 56, {"s0_pair": 6, "share": 1}, (), set(), range(6), ()),
    "FeatureExecutorBF16": ("feature", 50, {"share": 1}, (), set(), (), ()),
}


@pytest.fixture(scope="module")
def model():
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=48)), "cpu")
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    m.load_state_dict(sd, strict=True)
    return m.eval()


@pytest.fixture
def calls(monkeypatch):
    """kernels.pack_* as counting copies; CV_STEM off."""
    count = collections.Counter()

    def counting(name):
        def pack(w, *args):
            count[name] += 1
            return w.detach().clone()
        return pack

    for name in PACKERS:
        monkeypatch.setattr(kernels, name, counting(name))
    monkeypatch.setattr(ex, "CV_STEM", False)
    return count


def _conv_modules(net):
    from leastereo_amd.model import ConvBR
    return {name: mod for name, mod in net.named_modules() if isinstance(mod, ConvBR)}


def _w5(mod):
    """A ConvBR's weight as the 3D engines take it (a 2D 1x1 as one plane)."""
    w = mod.conv.weight
    return w.reshape(*w.shape[:2], 1, 1, 1) if w.dim() == 4 and w.shape[-1] == 1 else w


def _bn(mods):
    folded = [m.folded_bn() for m in mods]
    return torch.cat([f[0] for f in folded]), torch.cat([f[1] for f in folded])


def _expected(net, name, bf16, split_head):
    """(weight, scale, shift, relu) of entry ``name``, from the modules.  ``split_head``: the cell's
    sibling group runs as step 0's op (s1_group_head) + the rest (s1_group)."""
    parts = name.split(".")
    if name == "last_3.taps":
        w = net.last_3.conv.weight
        taps = w.permute(0, 2, 3, 4, 1).reshape(w.shape[0] * 27, w.shape[1], 1, 1, 1)
        if bf16:  # c8: 27 * cout channels padded to a block of 8
            taps = torch.cat([taps, taps.new_zeros(((-taps.shape[0]) % 8,) + tuple(taps.shape[1:]))], 0)
        return taps, None, None, False
    if parts[0] != "cells" or parts[2] in ("pre_preprocess", "preprocess", "_ops"):
        mod = net.get_submodule(name)
        return (_w5(mod),) + tuple(mod.folded_bn()) + (mod.relu,)
    i, kind = int(parts[1]), parts[2]
    cell = net.cells[i]
    if kind in ("s1_group", "s1_group_head"):
        ops = [op for _, op in GROUP]  # step order
        if split_head:
            ops = ops[:1] if kind == "s1_group_head" else ops[1:]
        mods = [cell._ops[op] for op in ops]
        return (torch.cat([m.conv.weight for m in mods], 0),) + _bn(mods) + (True,)
    if kind == "s0_pair":
        mods = [cell._ops[op] for _, op in S0_PAIR]
        return (torch.cat([m.conv.weight for m in mods], 0),) + _bn(mods) + (True,)
    if kind == "share":
        mods = [net.cells[i + 1].pre_preprocess, cell.preprocess]
        return (torch.cat([_w5(m) for m in mods], 0),) + _bn(mods) + (True,)
    if kind == "fanout":  # each head's BN / ReLU stay its own ConvBR's
        return torch.cat([_w5(cell.preprocess), _w5(net.cells[i + 1].pre_preprocess)], 0), None, None, False
    assert kind.startswith("pair"), name
    mods = [cell._ops[op] for op, _ in STEPS[int(kind[4:])]]
    # f32 (Winograd) packs [W_a | W_b] along cin; bf16 packs each half and concatenates the packs
    return (torch.cat([m.conv.weight for m in mods], 0 if bf16 else 1),) + _bn(mods) + (True,)


def _check_entries(e, net, bf16, f32_names=(), unlaunched=()):
    for name, p in e.p.items():
        head = name.rsplit(".", 1)[0] + ".s1_group_head" in e.p
        want_w, want_scale, want_shift, want_relu = _expected(net, name, bf16 and name not in f32_names, head)
        for got, want in ((p.scale, want_scale), (p.shift, want_shift)):
            assert (got is None) == (want is None), name
            assert want is None or torch.equal(got, want), name
        assert p.relu == want_relu, name
        cout, cin = want_w.shape[:2]
        if ".pair" in name and bf16:  # two [cout, cin] packs, one after the other
            cout, cin = cout // 2, 2 * cin
        assert (p.cout, p.cin, p.k) == (cout, cin, want_w.shape[-1]), name
        if name in unlaunched:
            continue
        got = p.wino if p.wino is not None else p.packed
        assert got.shape == want_w.shape and torch.equal(got, want_w), name


@pytest.mark.parametrize("cls", sorted(HOLDS))
def test_entries_plans_and_launch_weights(model, calls, cls):
    which, n_entries, stacked, group_cells, split, s0_cells, pair_cells = HOLDS[cls]
    net = getattr(model, which)
    e = getattr(ex, cls)(net)
    bf16 = cls.endswith("BF16")
    # the key set: every ConvBR, the stacked entries, and the matching head's taps
    want_keys = set(_conv_modules(net))
    cells = {"s1_group_head": sorted(split), "s1_group": list(group_cells), "s0_pair": list(s0_cells),
             "share": SHARE if which == "matching" else [3], "fanout": FANOUT,
             "pair0": list(pair_cells), "pair1": list(pair_cells), "pair2": list(pair_cells)}
    for kind, count in stacked.items():
        assert len(cells[kind]) == count
        want_keys |= {f"cells.{i}.{kind}" for i in cells[kind]}
    if which == "matching":
        want_keys.add("last_3.taps")
    assert set(e.p) == want_keys and len(e.p) == n_entries
    assert e.s1_group == {i: GROUP for i in group_cells}
    assert e.s1_split == split
    assert e.s0_pair == {i: S0_PAIR for i in s0_cells}
    assert e.pair_steps == {i: STEPS for i in pair_cells}
    # the f32 matching executor's 3x3x3 layers are the Winograd engine's (cin in chunks of 4); no other has any
    for name, p in e.p.items():
        assert (p.wino is not None) == (cls == "MatchingExecutor" and ex.WINOGRAD and p.k == 3 and p.cin % 4 == 0), name
    _check_entries(e, net, bf16, f32_names=("stem0", "stem1") if cls == "FeatureExecutorBF16" else (),
                   # bf16 matching: last_3 runs through last_3.taps + the tap-sum, its own weight is never launched
                   unlaunched=("last_3",) if cls == "MatchingExecutorBF16" else ())
    if which == "matching":
        assert e.cv is None and e.cv_win is None


def test_f32_pair_steps_stack_along_cin(model, calls, monkeypatch):
    """Not the default for f32 (LEASTEREO_PAIR_STEPS=1): the Winograd pair launch reads [W_a | W_b]."""
    monkeypatch.setattr(ex.MatchingExecutor, "PAIR_STEPS", True)
    e = ex.MatchingExecutor(model.matching)
    assert e.pair_steps == {i: STEPS for i in range(12)}
    assert sum(".pair" in name for name in e.p) == 36 and len(e.p) == 133 + 36
    _check_entries(e, model.matching, False)
    p = e.p["cells.0.pair1"]
    assert p.wino is not None and (p.cout, p.cin) == (16, 32) and p.scale.numel() == 32


# ---------------------------------------------- pack once, in the format that runs
def test_bf16_matching_makes_no_f32_pack(model, calls):
    ex.MatchingExecutorBF16(model.matching)
    assert not any(calls[name] for name in F32_PACKERS), dict(calls)
    assert calls["pack_conv_weight_bf16"] == 192 and calls["pack_conv2d_weight_bf16"] == 0


def test_bf16_feature_packs_f32_only_for_the_stems(model, calls):
    e = ex.FeatureExecutorBF16(model.feature)
    # stem0 (3 input channels) is the one f32 pack; the stride-3 stem1 launches with its raw weight
    assert {name: calls[name] for name in F32_PACKERS} == {"pack_conv_weight": 0, "pack_conv2d_weight": 1,
                                                           "pack_conv2d_weight_windowed": 0, "pack_conv_weight_wino": 0}
    assert e.p["stem0"].kind == "2d" and e.p["stem1"].kind == "s3"
    assert calls["pack_conv_weight_bf16"] == 17 and calls["pack_conv2d_weight_bf16"] == 31


def test_direct_builds_no_factored_stem(model, calls, monkeypatch):
    """With CV_STEM on: the direct executor reads the cost volume in place, so neither the weight
    split (a device kernel: it would raise here) nor the maps' packs run."""
    monkeypatch.setattr(ex, "CV_STEM", True)
    monkeypatch.setattr(kernels, "cv_stem_split_weights", lambda w: pytest.fail("factored-stem split"))
    e = ex.MatchingExecutorDirect(model.matching)
    assert e.cv is None and e.cv_win is None
    assert calls["pack_conv2d_weight"] == 0 and calls["pack_conv2d_weight_windowed"] == 0
    assert calls["pack_conv_weight"] == 121 and calls["pack_conv_weight_wino"] == 0
