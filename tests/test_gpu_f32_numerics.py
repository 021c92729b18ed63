"""Error bars of every fp32 conv dispatch path from a float32 model of its algorithm.

tests/test_gpu_parity.py and tests/test_gpu_wino.py hold the fp32 engines to |d| <= 1e-4 +
1e-4 |ref| on N(0,1) inputs: two to three decimal digits above what a correct float32 engine
does, so a Winograd constant typed with five digits passes there.  Here each path runs as a pure
convolution (no scale / shift, no ReLU, no residual) on the input cases of tests/f32_judge.py
(DC offsets, large magnitudes, a constant volume, an outlier voxel at three tile offsets, filters
that do not sum to zero) and must meet

    E(path) <= 4 x max(E(model of that path), E(direct_f32))     on the same inputs,

E = max |y - ref64| / S, S[b, co] = max conv(|x|, |w|), the model being the textbook float32
restatement of the algorithm the path's source states it computes (the table below).  4 x is the
project's margin over a float32 restatement (tests/test_gpu_disp_stats.py); the models sum one
product after another, the kernels in MFMA chunks of four channels with the transforms factored
differently (G's row constants applied to the accumulators: conv3d_wino.hip:21-25), E is a
maximum over ~1e5 outputs, and a short constant costs 5 to 48 x a model (test_f32_judge_cpu.py).  The
models meet E <= 2^-18 on every input used here (same file), so no bar exceeds 1.6e-5 of S.

A chain of four ConvBR layers and the disparity head ask the same question one step further.
Measured values: DESIGN.md, "fp32 engine numerics" (run with -s for the table).
"""

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels
from oracle import torch_ref as ref
from tests import f32_judge as J
from tests.f32_paths import PATHS, W44

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("path", sorted(PATHS))
def test_path_error_is_within_four_times_its_model(path):
    key, model, entry, settings, want_name, _, opts = PATHS[path]
    failures = []
    with _lib.tuning(**dict(settings)):
        for case, seed in J.INPUT_SETS:
            j = J.judged(key, case, seed)
            name, y = entry(j, **opts)
            assert name == want_name or (want_name[-1] in "< " and name.startswith(want_name)), (path, name)
            if path == "direct5_dp":  # the depth-paired direct tile (KD = 4)
                assert name.endswith(", 1, 4, false>"), name
            y = y.cpu().numpy()
            assert np.isfinite(y).all(), (path, case, seed)
            e, rel = j.error(y)
            em, ed, bar = j.e[model][0], j.e["direct"][0], j.bar(model)
            print(f"f32num {path:14s} {name} {key} {case} s{seed}: E {e:.2e} model {em:.2e} direct {ed:.2e} "
                  f"E/model {e / em:.2f} err/max|ref| {rel:.1e} bar {bar:.2e}")
            if not e <= bar:
                failures.append((case, seed, e, bar))
    assert not failures, (path, failures)


# ------------------------------------------------------------------ a chain of four ConvBR layers
CHAIN = {
    "direct": ("direct", (), "conv3d_dma_kernel<1, "),
    "wino42": ("wino42", ((W44, (0,)),), "conv3d_wino2_kernel<8, 1, 1, 4, 2, 5, false>"),
    "wino44": ("wino44", ((W44, (3,)),), "conv3d_wino44_kernel"),
}


@pytest.mark.parametrize("engine", sorted(CHAIN))
def test_chain_error_is_within_four_times_its_model(engine):
    """16 -> 16 -> 16 -> 16 -> 16 on (6, 9, 36): conv, a per-channel scale restoring unit
    variance, shift 0.1, ReLU; layers 2 and 4 add the chain's input (relu_dc activations, `normal`
    weights).  max |y - ref64| / max |ref64| within 4 x the same chain through the engine's model
    with float32 numpy epilogues."""
    model, settings, want_name = CHAIN[engine]
    x0, ws, scales, shifts, _ = J.chain_case()
    e_model = J.chain_error(J.chain_f32(lambda x, w: J.model(model, x, w)))
    c, shape = J.CHAIN_C, J.CHAIN_SHAPE
    with _lib.tuning(**dict(settings)):
        if engine == "direct":
            name = kernels.conv_kernel_name(1, c, *shape, 3)
        else:
            name = kernels.wino_kernel_name(1, c, *shape, cin=c)
        assert name == want_name or name.startswith(want_name), name
        xd = torch.from_numpy(x0).to(DEV)
        y = xd
        for l, w in enumerate(ws):
            wd, sc, sh = (torch.from_numpy(a).to(DEV) for a in (w, scales[l], shifts[l]))
            res = xd if l % 2 == 1 else None
            if engine == "direct":
                y = kernels.conv3d_bnrelu(y, kernels.pack_conv_weight(wd), c, 3, sc, sh, relu=True, residual=res)
            else:
                y = kernels.conv3d_bnrelu_wino(y, kernels.pack_conv_weight_wino(wd), c, sc, sh, relu=True,
                                               residual=res)
        y = y.cpu().numpy()
    assert np.isfinite(y).all()
    e = J.chain_error(y)
    print(f"f32num chain {engine} {name}: err/max|ref| {e:.2e} model {e_model:.2e} ratio {e / e_model:.2f}")
    assert e <= J.MARGIN * e_model, (engine, e, e_model)


# ------------------------------------------------------------------ disparity regression, plain entry
def _disp_cases(shape, seed):
    """Costs at gains 1, 3, 20, 60; the gain-20 costs + 1000 (the softmin must not care); one
    plane at 0 among planes at 50 (first, last, interior); an exact tie of two planes."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(shape, generator=g)
    d3 = shape[2]
    cases = {f"gain{k}": n * k for k in (1, 3, 20, 60)}
    cases["gain20+1000"] = n * 20 + 1000
    for tag, k in (("first", 0), ("last", d3 - 1), ("interior", d3 // 2 - 1)):
        c = torch.full(shape, 50.0)
        c[:, :, k] = 0
        cases["onehot_" + tag] = c
    c = torch.full(shape, 50.0)
    c[:, :, 1] = 0
    c[:, :, d3 - 3] = 0
    cases["tie"] = c
    return cases


@pytest.mark.parametrize("fast", [False, True], ids=["f32", "fastexp"])
@pytest.mark.parametrize("shape,md", [((1, 1, 16, 7, 4), 48), ((1, 1, 8, 5, 6), 24), ((2, 1, 32, 9, 13), 96)])
def test_disparity_forms_on_sharp_and_shifted_volumes(shape, md, fast):
    """kernels.disparity_regression, forms 0 .. 4 (lea_disparity_set_register_form), against
    oracle.torch_ref.disp_forward in float64.  f32: max error within max(4 x E_cpu, 32 ulp of
    maxdisp), E_cpu the float32 torch oracle's own error on that case; fast-exp: the project's
    bar (max 2e-3 px, mean 1e-4 px).  Form 4 multiplies exponentials of plane differences: the
    sharp volumes (gain 60, one-hot) are where that could underflow into 0 / 0."""
    failures = []
    for tag, x in _disp_cases(shape, 17 + md).items():
        want = ref.disp_forward(x.double(), md).numpy()
        e_cpu = float(np.abs(ref.disp_forward(x, md).double().numpy() - want).max())
        bar = max(J.MARGIN * e_cpu, 32 * float(np.spacing(np.float32(md))))
        for form in (0, 1, 2, 3, 4):
            with _lib.tuning(lea_disparity_set_register_form=form):
                y = kernels.disparity_regression(x.to(DEV), md, fast).cpu()
            assert torch.isfinite(y).all(), (tag, form, fast)
            err = np.abs(y.double().numpy() - want)
            print(f"f32num disp {shape} md{md} {'fastexp' if fast else 'f32'} form{form} {tag}: "
                  f"max {err.max():.2e} mean {err.mean():.2e} cpu32 {e_cpu:.2e} bar {bar:.2e}")
            ok = (err.max() < 2e-3 and err.mean() < 1e-4) if fast else err.max() <= bar
            if not ok:
                failures.append((tag, form, float(err.max()), float(err.mean()), bar))
    assert not failures, failures
