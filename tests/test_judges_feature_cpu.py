"""CPU checks of tests/feature_judge.py, the judge of tests/test_gpu_feature_exact.py.

Preconditions: every integer case the GPU file uses is exact on the reference (the case
constructors assert it; here each is built once without a GPU), the D = 1 embedding of a 2D conv in
f32_judge.direct_f32 is the 2D sum bit for bit, and on every normal case the float32 model costs
at most f32_judge.CAP (2^-18), so no 4 x bar exceeds 1.6e-5.

The judges reject planted defects.  Each defect is applied to the float64 reference in torch and
the GPU file's own check is shown to fail on it, in the int kind (not equal) and in the normal
kind (beyond 4 x the model; beyond half a bf16 ulp + 4 e32):
  a  a 2D conv whose left border tap is read clamped instead of zero
  b  stem1's padding ring filled with relu(shift0) instead of 0
  c  combine with the last-column correction taken one column off
  d  combine with the z = -1 term dropped
  e  truncation instead of round-to-nearest at a bf16 store
  f  a stride-3 conv reading rows 3 ho .. 3 ho + 2

How many of these defective outputs the bars of tests/test_gpu_parity.py and
tests/test_gpu_cv_stem.py would have passed on the same normal inputs (|d| <= 1e-4 + 1e-4 |ref| in
f32, 1e-5 for the stride-3 conv, 1e-2 + 1e-2 |ref| for the stems' c8 output, 1e-2 max |ref| for
stem0's) is OLD_BARS below, measured by old_bar_passes() and asserted to be current: none.
  a  0 of 14      b  0 of 4 in f32, 0 of 4 in c8      c  0 of 7 in f32, 0 of 4 in c8
  d  0 of 7 in f32, 0 of 4 in c8                       f  0 of 8
On N(0, 1) inputs a defect of the size of a whole tap or map term is beyond the old bars as well.
What they let through is smaller: test_old_bars_pass_a_single_wrong_pixel has one pixel of one
channel off by 5e-5, inside every old f32 bar and refused by the new ones in both kinds.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bf16_judge as B
from tests import f32_judge as F32
from tests import feature_judge as J

CONV2D = list(dict.fromkeys([(ci, co, hw, b) for ci, co in J.SMALL for hw, b in J.SMALL_SHAPES]
                            + [(ci, co, J.HW_RAGGED, 2) for ci, _, co in J.PAIR] + sorted(J.DMA2D)))
S3 = [(ci, co, hw) for ci, co in J.S3 for hw in J.S3_SHAPES]
OLD_BARS = {"a": (0, 14), "b f32": (0, 4), "b c8": (0, 4), "c f32": (0, 7), "c c8": (0, 4), "d f32": (0, 7),
            "d c8": (0, 4), "f": (0, 8)}


# ------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("cin,cout,hw,batch", CONV2D)
def test_conv2d_cases(cin, cout, hw, batch):
    c = J.conv2d_int(cin, cout, hw, batch)  # asserts its own exactness
    assert float(B.conv_raw(c["x"], c["w"], 3).abs().max()) > 0
    j = J.conv2d_normal(cin, cout, hw, batch)
    assert 0 < j.e_model <= J.CAP, j.e_model


@pytest.mark.parametrize("cin,cout,hw", S3)
def test_stride3_cases(cin, cout, hw):
    c = J.s3_int(cin, cout, hw)
    assert J.s3_judge(c["x"], c["w"], c["scale"], c["shift"], True).shape[2:] == ((hw[0] - 1) // 3 + 1,
                                                                                (hw[1] - 1) // 3 + 1)
    j = J.conv2d_normal(cin, cout, hw, 2, 3)
    assert 0 < j.e_model <= J.CAP, j.e_model


@pytest.mark.parametrize("hw", J.STEM_SHAPES)
def test_stem_cases(hw):
    c = J.stem_case("int", hw)  # asserts exactness and several positive shift0
    assert float(c["want"].max()) > 0 and c["e32"] == 0.0
    n = J.stem_case("normal", hw)
    peak = float(n["want"].abs().max())
    assert 0 < n["e_chain"] <= J.CAP and 0 < n["e32"] / peak <= J.CAP, (n["e_chain"], n["e32"])


@pytest.mark.parametrize("prec,key", [("f32", k) for k in J.CV_F32] + [("c8", k) for k in J.CV_C8])
def test_stem0_cases(prec, key):
    f = J.cv_case("int", prec, *key)  # asserts: maps exact in bf16, combine(maps) == the volume conv
    assert float(f["want"].max()) > 0
    n = J.cv_case("normal", prec, *key)
    if prec == "f32":
        assert 0 < max(n["e_comb"], n["e_direct"]) <= J.CAP
    else:
        peak = float(n["want"].abs().max())
        assert 0 < n["e32"] / peak <= J.CAP and 0 < n["e32_maps"] / float(n["lm"].abs().max()) <= J.CAP


def test_the_planes_split_where_the_cases_say():
    """cv_stem.hip's host code: dchunk = min(D3, (80 KB / 4 / ob - 191) / 2), ob = 16 (f32) / 32 (c8)."""
    for ob, d3 in ((16, J.CV_F32[-1][2] // 3), (32, J.CV_C8[-1][2] // 3)):
        dchunk = (80 * 1024 // 4 // ob - (3 * 64 - 1)) // 2
        assert d3 == dchunk + 1


def test_embedding_is_the_2d_sum_bit_for_bit():
    x, w = J.normal_conv2d(3, 5, 12, (9, 35))
    xp = F.pad(x, (1, 1, 1, 1))
    acc = torch.zeros(2, 12, 9, 35)
    for ci in range(5):
        for kh in range(3):
            for kw in range(3):
                acc += xp[:, ci:ci + 1, kh:kh + 9, kw:kw + 35] * w[:, ci, kh, kw].view(1, 12, 1, 1)
    assert np.array_equal(J.conv2d_f32_model(x, w), acc.numpy())
    x3, w3 = J.embed3d(x, w)
    np.testing.assert_allclose(F32.ref64(x3, w3, 3)[:, :, 0], J.conv2d_raw(x, w).numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(J.conv2d_f32_model(x, w, 3, torch.float64), J.conv2d_raw(x, w, 3).numpy(), rtol=0,
                               atol=1e-13)


# ------------------------------------------------------------------------------ planted defects
def clamped_left(x, w):
    """(a) the left border tap reads column 0 again instead of the zero padding."""
    xp = F.pad(x.double(), (1, 1, 1, 1))
    xp[..., 1:-1, 0] = x[..., 0].double()
    return F.conv2d(xp, w.double())


def rows_off(x, w):
    """(f) a stride-3 conv reading rows 3 ho .. 3 ho + 2 (the same number of outputs)."""
    return F.conv2d(F.pad(x.double(), (1, 1, 0, 2)), w.double(), None, 3, 0)


def ring_stem(c, dtype=torch.float64):
    """(b) stem1's padding ring holds relu(shift0): what stem0 makes of an all-zero patch."""
    a = J.stem0_act(c["x"], c["w0"], c["scale0"], c["shift0"], dtype)
    ring = torch.relu(c["shift0"].to(dtype)).view(1, -1, 1, 1).expand(a.shape[0], -1, a.shape[2] + 2, a.shape[3] + 2)
    ap = ring.clone()
    ap[..., 1:-1, 1:-1] = a
    return B.epilogue(F.conv2d(ap, c["w1"].to(dtype), None, 3, 0)[..., :(a.shape[2] - 1) // 3 + 1,
                                                                  :(a.shape[3] - 1) // 3 + 1],
                      c["scale1"], c["shift1"], True)


COMBINE_DEFECTS = {"c": dict(edge_shift=1), "d": dict(z_minus_1=False)}


def old_f32(y, ref, tol=1e-4):
    return bool(np.allclose(np.asarray(y, np.float64), np.asarray(ref, np.float64), rtol=tol, atol=tol))


def beyond_half_ulp(y64, want, e32):
    return B.half_ulp_stats(B.rn_bf16(y64), want, e32)["share"]


@pytest.mark.parametrize("cin,cout", J.SMALL)
def test_a_clamped_border_tap_is_rejected(cin, cout):
    c = J.conv2d_int(cin, cout, J.HW_RAGGED, 2)
    assert not torch.equal(clamped_left(c["x"], c["w"]), B.conv_raw(c["x"], c["w"], 3))
    j = J.conv2d_normal(cin, cout, J.HW_RAGGED, 2)
    assert j.error(clamped_left(j.x, j.w).numpy()) > j.bar


@pytest.mark.parametrize("hw", J.STEM_SHAPES)
def test_b_a_ring_of_relu_shift0_is_rejected(hw):
    c = J.stem_case("int", hw)
    bad = ring_stem(c)
    assert not torch.equal(bad, c["want"]) and int((bad != c["want"]).sum()) >= 4
    n = J.stem_case("normal", hw)
    bad = ring_stem(n)
    assert J.rel_error(bad.numpy(), n["want"].numpy()) > J.MARGIN * n["e_chain"]
    assert beyond_half_ulp(bad, n["want"], n["e32"]) > 0
    with pytest.raises(AssertionError):
        B.assert_half_ulp(B.rn_bf16(bad), n["want"], n["e32"])


@pytest.mark.parametrize("defect", sorted(COMBINE_DEFECTS))
@pytest.mark.parametrize("prec,key", [("f32", k) for k in J.CV_F32] + [("c8", k) for k in J.CV_C8])
def test_cd_a_wrong_combine_is_rejected(prec, key, defect):
    c, cout, maxdisp, hw, batch = key
    d3 = maxdisp // 3
    f = J.cv_case("int", prec, *key)
    lm, rm = J.stem0_maps(f["fl"], f["fr"], f["w"])
    bad = J.stem0_from_maps(lm, rm, cout, d3, f["scale"], f["shift"], **COMBINE_DEFECTS[defect])
    assert not torch.equal(bad, f["want"])
    n = J.cv_case("normal", prec, *key)
    lm, rm = J.stem0_maps(n["fl"], n["fr"], n["w"])
    if prec == "f32":
        bad = J.combine(lm, rm, cout, d3, **COMBINE_DEFECTS[defect])
        assert F32.error(bad.numpy(), n["ref"], n["s"])[0] > n["bar"]
    else:
        bad = J.stem0_from_maps(B.rn_bf16(lm), B.rn_bf16(rm), cout, d3, n["scale"], n["shift"],
                                **COMBINE_DEFECTS[defect])
        assert beyond_half_ulp(bad, n["want"], n["e32"]) > 0


def test_e_truncation_at_a_bf16_store_is_rejected():
    """At the output's store on 22-48 % of the elements (those whose nearest bf16 is the upper one;
    the ReLU's zeros are exact either way); at the maps' store on 28-30 %, and on 2 % of the split
    case, whose volume is mostly zero (W = 24 against D3 = 225)."""
    for hw in J.STEM_SHAPES:
        n = J.stem_case("normal", hw)
        assert B.half_ulp_stats(B.trunc_bf16(n["want"]), n["want"], n["e32"])["share"] > 0.1
        assert B.half_ulp_stats(B.rn_bf16(n["want"]), n["want"], n["e32"])["share"] == 0
    for key in J.CV_C8:
        n = J.cv_case("normal", "c8", *key)
        assert B.half_ulp_stats(B.trunc_bf16(n["want"]), n["want"], n["e32"])["share"] > 0.1
        assert B.half_ulp_stats(B.rn_bf16(n["want"]), n["want"], n["e32"])["share"] == 0
        # ... and at the maps' store: truncated maps move the output beyond the bar as well
        bad = J.stem0_from_maps(B.trunc_bf16(n["lm"]), B.trunc_bf16(n["rm"]), key[1], key[2] // 3, n["scale"],
                                n["shift"])
        assert beyond_half_ulp(bad, n["want"], n["e32"]) > 0.01


@pytest.mark.parametrize("cin,cout,hw", S3)
def test_f_rows_one_off_are_rejected(cin, cout, hw):
    c = J.s3_int(cin, cout, hw)
    assert not torch.equal(rows_off(c["x"], c["w"]), J.conv2d_raw(c["x"], c["w"], 3))
    j = J.conv2d_normal(cin, cout, hw, 2, 3)
    assert j.error(rows_off(j.x, j.w).numpy()) > j.bar


def old_bar_passes():
    """(passed, cases) per defect under the bars the per-op tests had before (module docstring)."""
    out = {}

    def count(key, flags):
        out[key] = (sum(flags), len(flags))
    count("a", [old_f32(clamped_left(j.x, j.w), j.ref) for j in
                (J.conv2d_normal(ci, co, J.HW_RAGGED, 2) for ci, co in J.SMALL)])
    stems = [(n, ring_stem(n)) for n in (J.stem_case("normal", hw) for hw in J.STEM_SHAPES)]
    count("b f32", [old_f32(bad, n["want"]) for n, bad in stems])
    count("b c8", [old_f32(B.rn_bf16(bad), n["want"], 1e-2) for n, bad in stems])
    for d, kw in COMBINE_DEFECTS.items():
        flags = []
        for key in J.CV_F32:
            n = J.cv_case("normal", "f32", *key)
            lm, rm = J.stem0_maps(n["fl"], n["fr"], n["w"])
            flags.append(old_f32(J.combine(lm, rm, key[1], key[2] // 3, **kw), n["ref"]))
        count(d + " f32", flags)
        flags = []
        for key in J.CV_C8:
            n = J.cv_case("normal", "c8", *key)
            want = B.costvolume_judge(n["fl"], n["fr"], key[2], n["w"], n["scale"], n["shift"], True)
            bad = B.rn_bf16(J.stem0_from_maps(B.rn_bf16(n["lm"]), B.rn_bf16(n["rm"]), key[1], key[2] // 3,
                                              n["scale"], n["shift"], **kw))
            flags.append(float((bad - want).abs().max()) <= 1e-2 * float(want.abs().max()))
        count(d + " c8", flags)
    count("f", [old_f32(rows_off(j.x, j.w), j.ref, 1e-5) for j in
                (J.conv2d_normal(ci, co, hw, 2, 3) for ci, co, hw in S3)])
    return out


def test_old_bar_counts_are_current():
    assert old_bar_passes() == OLD_BARS


def test_old_bars_pass_a_single_wrong_pixel():
    """One output of one channel off by 5e-5 (a seam pixel, say): inside 1e-4 + 1e-4 |ref|, outside
    4 x the float32 model; on the integer recipe any change at all is refused."""
    j = J.conv2d_normal(8, 12, J.HW_RAGGED, 2)
    bad = j.ref.copy()
    bad[1, 3, 8, 32] += 5e-5
    assert old_f32(bad, j.ref) and j.error(bad) > j.bar
    n = J.stem_case("normal", (23, 200))
    bad = n["want"].clone()
    bad[1, 3, 4, 64] += 5e-5
    assert old_f32(bad, n["want"]) and J.rel_error(bad.numpy(), n["want"].numpy()) > J.MARGIN * n["e_chain"]
