"""Whole model with the work-skipping routes of the f32 matching executor on and off, alone and
together: the two-head 1x1 (MatchingExecutor.FANOUT_1X1) and stem0's windowed 2D maps
(MatchingExecutor.WINDOWED_MAPS).  The routes merge or skip launches' work and change no
arithmetic, so the disparity is compared with torch.equal.

Shapes: the golden e2e case (96 x 192, D 48), and 288 x 576, D 96, where cell 10's down route
(its s1 through lea_resample3d_trilinear_down2) takes its raw z from the two-head launch."""
import pytest
import torch

from leastereo_amd import executor, kernels
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from tests.golden_util import normal, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _forward(m, left, right, fanout, windowed=False):
    old = executor.MatchingExecutor.FANOUT_1X1, executor.MatchingExecutor.WINDOWED_MAPS
    executor.MatchingExecutor.FANOUT_1X1, executor.MatchingExecutor.WINDOWED_MAPS = fanout, windowed
    try:
        m.matching.invalidate()  # the plan is made when the executor is built
        with torch.no_grad(), kernels.KernelProbe() as probe:
            disp = m(left, right)
        return disp, [(r.name, r.shape) for r in probe.records]
    finally:
        executor.MatchingExecutor.FANOUT_1X1, executor.MatchingExecutor.WINDOWED_MAPS = old
        m.matching.invalidate()


def _plain_1x1(recs):
    """(cin, cout) of every launch of the single-output streaming 1x1."""
    return sorted(s[1:3] for n, s in recs if n.startswith("conv1x1_kernel<"))


@pytest.mark.parametrize("height,width,maxdisp,down_route", [(96, 192, 48, False), (288, 576, 96, True)])
def test_disparity_is_equal_with_the_route_on_and_off(height, width, maxdisp, down_route):
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=maxdisp)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    m = m.to(DEV).eval()
    left, right = normal(931, (1, 3, height, width)).to(DEV), normal(932, (1, 3, height, width)).to(DEV)
    on, recs = _forward(m, left, right, True)
    off, recs0 = _forward(m, left, right, False)
    assert torch.equal(on, off)
    assert not on.isnan().any()
    # six two-head launches, one per pair; each replaces the pair's two single launches
    heads = [s[1:3] for n, s in recs if n.startswith("conv1x1_heads_kernel<")]
    assert sorted(heads) == sorted([(128, 48), (128, 48), (128, 64), (128, 48), (64, 24), (64, 24)])
    assert not [n for n, _ in recs0 if n.startswith("conv1x1_heads_kernel<")]
    assert len(recs) == len(recs0) - 6
    gone = _plain_1x1(recs0)
    for cio in _plain_1x1(recs):
        gone.remove(cio)
    assert gone == sorted([(128, 32), (128, 16)] * 3 + [(128, 32)] * 2 + [(64, 16), (64, 8)] * 2)
    names = [n for n, _ in recs]
    assert ("resample3d_sep_down2_f32" in names) == down_route
    # the windowed maps, alone and with the two-head route: the two map launches become windowed ones
    for fanout in (False, True):
        win, recsw = _forward(m, left, right, fanout, True)
        assert torch.equal(win, off)
        assert len([n for n, _ in recsw if n.endswith(" windowed")]) == 2
        assert len(recsw) == len(recs if fanout else recs0)
    assert not [n for n, _ in recs + recs0 if n.endswith(" windowed")]
