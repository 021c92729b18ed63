"""What one cell hands the next -- the level-down copy of its output, the next cell's precomputed
s0 -- travels in cell()'s result and arguments, not on the executor: a forward leaves no tensor
referenced from the executor, whether it returns or raises half way.  On the CPU, float64, with the
torch stand-ins of tests/executor_stands.py."""
import dataclasses

import pytest
import torch

from leastereo_amd import executor as ex
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from leastereo_amd.weights import synthetic_state_dict
from tests.executor_stands import Stand
from tests.golden_util import normal


class Boom(RuntimeError):
    pass


class RaisingStand(Stand):
    """Raises at the first 3x3x3 conv after a stacked down-sampling 1x1 (cells.0.share, the first
    resampled conv of a forward): a step conv of cell 0, after that cell's ``share`` launch."""

    def __init__(self, armed):
        super().__init__()
        self.armed, self.shared = armed, False

    def conv3d_bnrelu_resampled(self, *args, **kw):
        self.shared = True
        return super().conv3d_bnrelu_resampled(*args, **kw)

    def conv3d_bnrelu(self, x, packed, cout, k, *args, **kw):
        if self.armed and self.shared and k == 3:
            raise Boom(f"step conv, cout {cout}")
        return super().conv3d_bnrelu(x, packed, cout, k, *args, **kw)


def _tensors(root):
    """ids of every tensor reachable from ``root`` through containers, dataclasses and objects'
    attributes (modules included: their parameter and buffer dicts are attributes)."""
    seen, found, todo = set(), set(), [root]
    while todo:
        o = todo.pop()
        if id(o) in seen or isinstance(o, (str, bytes, int, float, bool, type(None), type)):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            found.add(id(o))
            todo.append(o.grad)
        elif isinstance(o, dict):
            todo.extend(o.keys())
            todo.extend(o.values())
        elif isinstance(o, (list, tuple, set, frozenset)):
            todo.extend(o)
        elif dataclasses.is_dataclass(o) or hasattr(o, "__dict__"):
            todo.extend(vars(o).values())
    return found


@pytest.mark.parametrize("raises", [True, False])
def test_a_forward_leaves_no_tensor_on_the_executor(monkeypatch, raises):
    st = RaisingStand(raises).install(monkeypatch)
    monkeypatch.setattr(ex, "CV_STEM", False)
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=48)), "cpu")
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, bn_file=None)
    m.load_state_dict(sd, strict=True)
    m = m.double().eval()
    me = ex.MatchingExecutor(m.matching)
    assert "cells.0.share" in me.p
    before = _tensors(vars(me))  # (all kept alive by the executor: no id below is a reused one)
    x = normal(903, (1, 64, 16, 32, 64)).double()
    with torch.no_grad():
        if raises:
            with pytest.raises(Boom):
                me.run(x)
            assert st.shared, "the share launch ran before the step conv that raised"
        else:
            assert me.run(x).shape == (1, 1, 16, 32, 64)
    left = _tensors(vars(me)) - before
    assert not left, f"{len(left)} tensor(s) left on the executor: {sorted(k for k, v in vars(me).items() if _tensors(v) - before)}"
