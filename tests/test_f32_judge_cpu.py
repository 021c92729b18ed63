"""The float32 judge judged (tests/f32_judge.py; no GPU): its Winograd model is the convolution
(exact in float64), every model it lends to tests/test_gpu_f32_numerics.py costs at most 2^-18 of
S on every input that test uses (the precondition under which 4 x a model is a tight bar), and
that bar does fail -- on a Winograd constant typed with five digits and on 1e-5 S at one voxel."""
import numpy as np
import pytest
import torch

from tests import f32_judge as J


@pytest.mark.parametrize("fw,fd", [(2, 1), (4, 1), (2, 2), (4, 2), (4, 4)])
@pytest.mark.parametrize("shape,cin,cout,batch", [((7, 5, 10), 6, 5, 2), ((5, 3, 13), 3, 4, 2), ((1, 1, 1), 1, 1, 1)])
def test_wino_model_is_exact_in_float64(fw, fd, shape, cin, cout, batch):
    """Ragged volumes (W and D no multiples of 4 or 2), cin no multiple of 4, batch 2."""
    x, w = J.inputs("normal", 3, shape, cin, cout, batch)
    ref, s = J.ref64(x, w, 3), J.scale(x, w)
    for kw in ({}, {"pairwise": True}):
        e, _ = J.error(J.wino_f32(x, w, fw, fd, dtype=torch.float64, **kw), ref, s)
        assert e <= 1e-12, (kw, e)
    assert J.error(J.direct_f32(x, w, 3, dtype=torch.float64), ref, s)[0] <= 1e-12


def test_direct_model_k1_is_exact_in_float64():
    x, w = J.inputs("relu_dc", 1, (3, 4, 5), 7, 3, 2, k=1)
    assert J.error(J.direct_f32(x, w, 1, dtype=torch.float64), J.ref64(x, w, 1), J.scale(x, w))[0] <= 1e-12


def test_input_cases():
    shape, cin, cout = (5, 4, 12), 8, 3
    xn, wn = J.inputs("normal", 2, shape, cin, cout)
    assert xn.dtype == np.float32 and wn.dtype == np.float32 and xn.shape == (1, cin) + shape
    assert abs(float(wn.std()) * np.sqrt(27 * cin) - 1) < 0.1
    x, w = J.inputs("relu_dc", 2, shape, cin, cout)
    assert x.min() == 0 and x.mean() > 3 and np.array_equal(w, wn)
    assert np.array_equal(J.inputs("x100", 2, shape, cin, cout)[0], xn * np.float32(100))
    assert (J.inputs("const", 2, shape, cin, cout)[0] == np.float32(7.3)).all()
    x, w = J.inputs("wmean", 2, shape, cin, cout)
    assert np.array_equal(x, xn) and np.array_equal(w, wn + np.float32(0.05))
    x, w = J.inputs("relu_dc_wmean", 2, shape, cin, cout)
    assert np.array_equal(x, J.inputs("relu_dc", 2, shape, cin, cout)[0]) and np.array_equal(w, wn + np.float32(0.05))
    offs = set()
    for seed in range(3):
        x, _ = J.inputs("spike", seed, shape, cin, cout)
        ci, d, h, wq = J.spike_voxel(seed, shape, cin)
        assert x[0, ci, d, h, wq] == np.float32(J.SPIKE) and np.sum(np.abs(x) > 0.1) == 1
        assert d % 4 == wq % 4
        offs.add(wq - 4)
    assert offs == {0, 3, 4}  # a tile's first and last output, and the next tile's first (the halo)


@pytest.mark.parametrize("key", sorted(J.TUPLES))
def test_models_meet_the_precondition(key):
    """A condition, not a measurement: E(model) <= 2^-18 for every model and input set the GPU
    test uses.  (Prints the table of DESIGN.md, "fp32 engine numerics", with -s.)"""
    for case, seed in J.INPUT_SETS:
        j = J.judged(key, case, seed)
        print(f"f32judge {key:8s} {case:13s} s{seed} " +
              " ".join(f"{m} {e:.2e} ({r:.1e})" for m, (e, r) in j.e.items()))
        for m, (e, _) in j.e.items():
            assert e <= J.CAP, (key, case, seed, m, e)


@pytest.mark.parametrize("name,key", [("wino44", "c32x32"), ("wino42", "c32x32"), ("wino44", "c128x64"),
                                      ("wino42", "c32x96")])
@pytest.mark.parametrize("case", ["normal", "relu_dc"])
def test_a_five_digit_sixth_fails_the_bar(name, key, case):
    """G's 1/6 typed as 0.16667 (3.3e-6 off, 2e-5 relative) must miss 4 x E(wino_f32)."""
    j = J.judged(key, case, 0)
    e_bad, _ = j.error(J.model(name, j.x, j.w, sixth=0.16667))
    print(f"f32judge planted 0.16667 {name} {key} {case}: E {e_bad:.2e} vs model {j.e[name][0]:.2e}, "
          f"bar {j.bar(name):.2e}")
    assert e_bad > J.MARGIN * j.e[name][0] and e_bad > j.bar(name)


@pytest.mark.parametrize("key", sorted(J.TUPLES))
def test_one_voxel_off_by_1e5_s_fails_the_bar(key):
    """A correct result (float64 rounded to float32) with 1e-5 S added at one voxel misses
    4 x E(wino_f32) of every Winograd model of the tuple, and the GPU test's bar, on `normal` and
    `relu_dc` (where a model costs at most 2.5e-6; at the 2^-18 cap the bar is 1.5e-5)."""
    for case in ("normal", "relu_dc"):
        j = J.judged(key, case, 0)
        y = j.ref.astype(np.float32)
        b, co = y.shape[0] - 1, y.shape[1] // 2
        y[b, co, 1, 2, 3] += np.float32(1e-5 * j.s[b, co])
        e, _ = j.error(y)
        for m in j.e:
            assert e > j.bar(m) and e > J.MARGIN * j.e[m][0], (key, case, m, e, j.bar(m))


def test_sequential_sums_are_the_least_favourable_order():
    """Pairwise against sequential channel sums: the tree sum is the more exact one (by up to
    4.5 x here, on F(4,3) along W with its 288 terms), so a bar of 4 x the sequential model has
    room for any order of the kernels' MFMA chunks, and a model is no tighter than a kernel can be."""
    for name, key in (("wino44", "c32x32"), ("wino42", "c32x32"), ("wino22", "c16x16"), ("wino41", "c32x32r")):
        for case in ("normal", "relu_dc", "relu_dc_wmean"):
            j = J.judged(key, case, 0)
            e_pair, _ = j.error(J.model(name, j.x, j.w, pairwise=True))
            r = e_pair / j.e[name][0]
            print(f"f32judge order {name} {key} {case}: pairwise / sequential {r:.2f}")
            assert r < 1.5


def test_chain_models():
    """The four-layer chain through each model: finite, and its error against the float64 chain
    is what the GPU chain test multiplies by 4."""
    x0, ws, scales, shifts, ref = J.chain_case()
    assert len(ws) == len(scales) == len(shifts) == 4 and np.isfinite(ref).all() and ref.std() > 0.5
    for name in ("direct", "wino42", "wino44"):
        y = J.chain_f32(lambda x, w: J.model(name, x, w))
        e = J.chain_error(y)
        print(f"f32judge chain {name}: err / max|ref| {e:.2e}")
        assert np.isfinite(y).all() and 0 < e < 1e-5
