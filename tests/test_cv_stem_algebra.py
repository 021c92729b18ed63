"""CPU check of the algebra behind csrc/cv_stem.hip: stem0's 3x3x3 conv over the cost
volume (retrain/LEAStereo.py:34-48, skip_model_3d.py:141) equals the per-plane sum of
2D maps the factored kernel combines (include/leastereo_hip.h, lea_cv_stem_combine).
Float64 torch on CPU: the identity is exact up to summation order."""
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as ref
from tests.feature_judge import combine, split_weights


@pytest.mark.parametrize("b,c,cout,maxdisp,hw", [(1, 4, 8, 27, (5, 8)), (2, 3, 4, 48, (4, 21)),
                                                  (1, 2, 3, 6, (3, 4)), (1, 4, 4, 9, (6, 3)),
                                                  (1, 3, 5, 24, (2, 30))])
def test_factored_stem_equals_the_cost_volume_conv(b, c, cout, maxdisp, hw):
    g = torch.Generator().manual_seed(b * 100 + c * 10 + cout)
    fl = torch.randn((b, c) + hw, generator=g, dtype=torch.float64)
    fr = torch.randn((b, c) + hw, generator=g, dtype=torch.float64)
    w = torch.randn(cout, 2 * c, 3, 3, 3, generator=g, dtype=torch.float64)
    d3 = int(maxdisp / 3)
    want = F.conv3d(ref.build_cost_volume(fl, fr, maxdisp), w, None, 1, 1)
    wl, wr = split_weights(w)
    lm = F.conv2d(fl, wl, None, 1, 1)
    rm = F.conv2d(fr, wr, None, 1, 1)
    got = combine(lm, rm, cout, d3)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
