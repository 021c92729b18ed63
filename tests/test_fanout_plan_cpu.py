"""The two-head 1x1 route of the matching executor (MatchingExecutor.FANOUT_1X1), checked on the
CPU: which (cell i ``preprocess``, cell i + 1 ``pre_preprocess``) pairs are planned as one
launch, and that the graph the executor then runs -- this cell's head in its slot or through the
commuted up-sampling, the next cell's head handed over in the share memo -- is still
newMatching.forward.

In the manner of tests/test_executor_plan_cpu.py: the launches are replaced by torch ops with
the same contract (here including lea_conv1x1_heads) and the executor runs in float64 on CPU
tensors against the oracle.  The route is an f32 device route, so this test forces it on through
``_fanout_takes``; without that no CPU tensor takes it.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from leastereo_amd import executor as ex
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from leastereo_amd.weights import synthetic_state_dict
from oracle import torch_ref as ref
from tests.executor_stands import Stand, _act, _emit
from tests.golden_util import arch, normal


class HeadsStand(Stand):
    """+ the two-head 1x1 (lea_conv1x1_heads)."""

    def __init__(self):
        super().__init__()
        self.heads = []   # (source data_ptr, cout_a, head A has BN, cout_b, head B has BN)

    def conv3d_bnrelu_wino(self, *args, pair_sum=False, **kw):
        assert not pair_sum  # (PAIR_STEPS is off on this path)
        return super().conv3d_bnrelu_wino(*args, **kw)

    def conv1x1_heads(self, x, packed, cout_a, scale_a, shift_a, relu_a, cout_b, scale_b, shift_b, relu_b,
                      out_a=None, out_b=None, x2=None):
        assert packed.shape[0] == cout_a + cout_b and x2 is None
        self.heads.append((x.data_ptr(), cout_a, scale_a is not None, cout_b, scale_b is not None))
        z = F.conv3d(x, packed.to(x.dtype))
        return (_emit(_act(z[:, :cout_a], scale_a, shift_a, relu_a), out_a),
                _emit(_act(z[:, cout_a:], scale_b, shift_b, relu_b), out_b))


@pytest.fixture
def stand(monkeypatch):
    st = HeadsStand().install(monkeypatch, extra=("conv1x1_heads",))
    monkeypatch.setattr(ex, "CV_STEM", False)
    monkeypatch.setattr(ex.MatchingExecutor, "PAIR_STEPS", False)
    return st


def _matching(tmp_path, path=None):
    args = LEAStereoArgs(maxdisp=48)
    a = arch()
    if path is not None:
        a["net_arch_mat"] = np.array(path)
        args.mat_num_layers = len(path)
        args.net_arch_mat = str(tmp_path / "mat_path.npy")
        np.save(args.net_arch_mat, a["net_arch_mat"])
    m = LEAStereo(default_arch_args(args), "cpu")
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    m.load_state_dict(sd, strict=True)
    return m.double().eval(), sd, a


def _planned(me, key):
    return sorted(int(k.split(".")[1]) for k in me.p if k.endswith("." + key))


# the shipped 12-cell path, and a 5-cell one that only goes down (no conv1 / conv2, no up-sampling)
PATHS = {"shipped": (None, [3, 4, 6, 7, 9, 10], [0, 2, 5, 8]), "down_only": ([1, 1, 2, 2, 2], [3], [0, 2])}


@pytest.mark.parametrize("name", sorted(PATHS))
@pytest.mark.parametrize("on", [True, False])
def test_fanout_plan_matches_oracle(tmp_path, stand, monkeypatch, name, on):
    path, fanout, share = PATHS[name]
    monkeypatch.setattr(ex.MatchingExecutor, "FANOUT_1X1", on)
    monkeypatch.setattr(ex.MatchingExecutor, "_fanout_takes", lambda self, x: True)
    m, sd, a = _matching(tmp_path, path)
    me = ex.MatchingExecutor(m.matching)
    assert _planned(me, "fanout") == (fanout if on else [])
    assert _planned(me, "share") == share  # cells.{i}.share is what it was
    x = normal(903, (1, 64, 16, 32, 64)).double()
    with torch.no_grad():
        got = me.run(x)
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        want = ref.matching_forward(sd64, x, a["net_arch_mat"], a["cell_arch_mat"])
    assert len(stand.heads) == (len(fanout) if on else 0)
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    # folded BN is f32 by design: ~1e-7 relative per layer; a plan error is O(1)
    assert err <= 1e-5 * float(want.abs().max()), err
    if on:
        # no source of a two-head launch is read by a single 1x1 as well
        assert not {h[0] for h in stand.heads} & {s[0] for s in stand.single}
    if on and name == "shipped":
        # heads (own, next) per planned cell: BN on a head = plain, none = the commuted up-sampling's raw z
        assert [h[1:] for h in stand.heads] == [(32, True, 16, False), (16, False, 32, True), (32, True, 32, True),
                                                 (32, True, 16, False), (16, True, 8, False), (8, False, 16, True)]


def test_cpu_tensors_do_not_take_the_route(tmp_path, stand, monkeypatch):
    """Planned, but never taken off the device: the launches are today's."""
    monkeypatch.setattr(ex.MatchingExecutor, "FANOUT_1X1", True)
    m, _, _ = _matching(tmp_path, [1, 1, 2, 2, 2])
    me = ex.MatchingExecutor(m.matching)
    assert _planned(me, "fanout") == [3]
    with torch.no_grad():
        me.run(normal(5, (1, 64, 8, 16, 32)).double())
    assert not stand.heads


def test_other_executors_do_not_plan_it():
    assert not ex.CellGraphExecutor.FANOUT_1X1 and not ex.FeatureExecutor.FANOUT_1X1
    assert not ex.MatchingExecutorDirect.FANOUT_1X1 and not ex.MatchingExecutorBF16.FANOUT_1X1
