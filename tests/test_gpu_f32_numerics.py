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

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _direct(j, split=0, **_):
    x, w = torch.from_numpy(j.x).to(DEV), torch.from_numpy(j.w).to(DEV)
    cout, k = w.shape[0], w.shape[-1]
    name = kernels.conv_kernel_name(x.shape[0], cout, *x.shape[2:], k)
    x1, x2 = (x[:, :split].contiguous(), x[:, split:].contiguous()) if split else (x, None)
    y = kernels.conv3d_bnrelu(x1, kernels.pack_conv_weight(w), cout, k, None, None, relu=False, x2=x2)
    return name, y


def _wino(j, pair=False, **_):
    x, w = torch.from_numpy(j.x).to(DEV), torch.from_numpy(j.w).to(DEV)
    cout, cin = w.shape[0], w.shape[1]
    packed = kernels.pack_conv_weight_wino(w)
    if pair:  # LEA_PAIR_SUM: always the F(2,3) x F(2,3) tile (csrc/conv3d_wino.hip:1023-1026)
        xa, xb = x[:, :cin // 2].contiguous(), x[:, cin // 2:].contiguous()
        out = torch.empty((x.shape[0], cout) + tuple(x.shape[2:]), device=DEV)
        assert kernels.pair_sum_supported(xa, xb, out)
        return "conv3d_wino22_kernel", kernels.conv3d_bnrelu_wino(xa, packed, cout, None, None, relu=False,
                                                                   out=out, x2=xb, pair_sum=True)
    name = kernels.wino_kernel_name(x.shape[0], cout, *x.shape[2:], cin=cin)
    return name, kernels.conv3d_bnrelu_wino(x, packed, cout, None, None, relu=False)


W44 = "lea_conv3d_wino44_set"
TILE = "lea_conv3d_wino_set_tile_override"
# id: (tuple of f32_judge.TUPLES, model, entry, settings, kernel name (exact, or a prefix ending
#      in "<" / ", "), the csrc line that states which algorithm the kernel computes, entry options)
PATHS = {
    # direct MFMA engine, k = 3: couts 16 / 32 / 64 (the last with two sources)
    "direct16": ("c16x16", "direct", _direct, (), "conv3d_dma_kernel<1, ", "conv3d.hip:603,743", {}),
    "direct32": ("c32x32", "direct", _direct, (), "conv3d_dma_kernel<2, ", "conv3d.hip:603,743", {}),
    "direct64_x2": ("c128x64", "direct", _direct, (), "conv3d_dma_kernel<4, ", "conv3d.hip:603,743", {"split": 64}),
    # small couts: the VALU engine (couts 1, 2) and the depth-paired MFMA tile (couts 3 .. 8)
    "valu1": ("c16x1", "direct", _direct, (), "conv3d_valu_kernel<1>", "conv3d.hip:587-588", {}),
    "valu2": ("c16x2", "direct", _direct, (), "conv3d_valu_kernel<2>", "conv3d.hip:587-588", {}),
    "direct5_dp": ("c16x5", "direct", _direct, (), "conv3d_dma_kernel<1, ", "conv3d.hip:594-595,746", {}),
    # 1x1x1, one float per lane and NT-float vectors
    "conv1x1_scalar": ("k1c128", "direct", _direct, (("lea_conv1x1_set_vector", (0,)),), "conv1x1_kernel<2, ",
                       "conv3d.hip:579-580", {}),
    "conv1x1_vector": ("k1c128", "direct", _direct, (("lea_conv1x1_set_vector", (1,)),), "conv1x1_kernel<2, ",
                       "conv3d.hip:579-580", {}),
    # 1-D Winograd along W: F(2,3), F(4,3) on 64-wide rows, F(4,3) on 32-wide row pairs (f = 8)
    "wino1d_f2": ("c32x32r", "wino21", _wino, ((TILE, (1, 2, 2)),), "conv3d_wino_kernel<2, 16, 2, 1, 2, false>",
                  "conv3d_wino.hip:9-11,877-878", {}),
    "wino1d_f4": ("c32x32r", "wino41", _wino, ((TILE, (1, 1, 4)),), "conv3d_wino_kernel<4, 16, 2, 1, 1, false>",
                  "conv3d_wino.hip:12-16,877-878", {}),
    "wino1d_f8": ("c32x32r", "wino41", _wino, ((TILE, (1, 2, 8)),), "conv3d_wino_kernel<4, 8, 2, 1, 2, false>",
                  "conv3d_wino.hip:12-16,877-878", {}),
    # depth-paired tile, couts <= 8: F(4,3) along W, direct along D (the F of the kernel name)
    "wino_dp8": ("c8x8w", "wino41", _wino, (), "conv3d_wino_kernel<4, 16, 0, 1, 2, false, true, true>",
                 "conv3d_wino.hip:881-882", {}),
    "wino_dp4": ("c8x4", "wino41", _wino, (), "conv3d_wino_kernel<4, 8, 0, 1, 2, false>",
                 "conv3d_wino.hip:881-882", {}),
    # F(4,3) along W x F(2,3) along D, the one-barrier pipeline
    "wino2p_32": ("c32x32", "wino42", _wino, ((W44, (0,)),), "conv3d_wino2p_kernel", "conv3d_wino2.hip:1-12", {}),
    "wino2p_96": ("c32x96", "wino42", _wino, ((W44, (0,)),), "conv3d_wino2p_kernel", "conv3d_wino2.hip:1-12", {}),
    # the per-lane W x D kernel (16 couts): 16-byte halo pieces (the default) and dword pieces
    "wino2_lane": ("c16x16", "wino42", _wino, (("lea_conv3d_wino_set_variant", (0,)),),
                   "conv3d_wino2_kernel<8, 1, 1, 4, 2, 5, false>", "conv3d_wino2.hip:1-12", {}),
    "wino2_lane_v2": ("c16x16r", "wino42", _wino, (("lea_conv3d_wino_set_variant", (2,)),),
                      "conv3d_wino2_kernel<8, 1, 1, 4, 2, 0, false>", "conv3d_wino2.hip:1-12", {}),
    # F(4,3) x F(4,3): modes 1 (couts 32 / 64), 2 (cin 8, cout 24), 3 (cout 16)
    "wino44_32": ("c32x32", "wino44", _wino, ((W44, (1,)),), "conv3d_wino44_kernel", "conv3d_wino44.hip:1-9", {}),
    "wino44_64": ("c128x64", "wino44", _wino, ((W44, (1,)),), "conv3d_wino44_kernel", "conv3d_wino44.hip:1-9", {}),
    "wino44_24": ("c8x24", "wino44", _wino, ((W44, (2,)),), "conv3d_wino44_kernel", "conv3d_wino44.hip:1-9", {}),
    "wino44_16": ("c16x16", "wino44", _wino, ((W44, (3,)),), "conv3d_wino44_kernel", "conv3d_wino44.hip:1-9", {}),
    # F(2,3) x F(2,3): the 16-cout tile, and LEA_PAIR_SUM against the sum of two models
    "wino22_16": ("c16x16", "wino22", _wino, (("lea_conv3d_wino_set_w22", (1,)),), "conv3d_wino22_kernel",
                  "conv3d_wino22.hip:3", {}),
    "wino22_pair": ("p32x16", "pair22", _wino, (), "conv3d_wino22_kernel", "conv3d_wino22.hip:3,193-202",
                    {"pair": True}),
}


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
