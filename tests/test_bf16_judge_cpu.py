"""The bf16 judge (tests/bf16_judge.py) judged on the CPU: it accepts a correctly rounded
float32 restatement with no failing element, and rejects wrong answers -- among them two
rounding defects that the older per-op bar of tests/test_gpu_bf16.py (max |d| <= 1e-2 x
max |ref| over the tensor) accepts, which is the gap the half-ulp and integer checks close."""
import functools

import pytest
import torch

from tests import bf16_judge as J

# the existing case recipes of test_conv_bf16_vs_torch (b, cin, cout, k, shape), its seeds
RECIPES = [(1, 64, 32, 3, (6, 20, 70)), (1, 128, 32, 1, (2, 5, 33)), (1, 8, 8, 3, (5, 9, 40))]
K128 = (1, 128, 64, 3, (4, 9, 21))  # the largest K used on the GPU (cin 128, k 3)


def old_close(got, want, rel=1e-2):
    """_close of tests/test_gpu_bf16.py, as a predicate."""
    got, want = got.double(), want.double()
    return float((got - want).abs().max()) <= rel * (float(want.abs().max()) + 1e-6)


@functools.lru_cache(None)
def normal_ref(b, cin, cout, k, shape):
    c = J.normal_case(cin * 13 + cout + k, cin, cout, k, shape, b)
    j64 = J.conv_judge(c["x"], c["w"], c["scale"], c["shift"], True, k=k)
    j32 = J.conv_judge(c["x"], c["w"], c["scale"], c["shift"], True, k=k, dtype=torch.float32)
    return c, j64, j32, J.e32_of(j32, j64)


@functools.lru_cache(None)
def pair_ref(c, shape):
    p = J.normal_pair_case(c * 3 + shape[0], c, shape)
    args = (p["xa"], p["wa"], p["xb"], p["wb"], p["sc"], p["sh"])
    a64, b64 = J.pair_terms(*args)
    e32 = J.e32_of(J.pair_judge(*args, False, dtype=torch.float32), a64 + b64)
    return args, a64, b64, e32


def rejected(got, want64, e32, alts=()):
    with pytest.raises(AssertionError):
        J.assert_half_ulp(got, want64, e32, alts)
    return J.half_ulp_stats(got, want64, e32, alts)["share"]


def test_rn_bf16_is_torchs_rounding_and_ulp_is_the_spacing():
    g = torch.Generator().manual_seed(0)
    x = torch.cat((torch.randn(4096, generator=g) * 3, torch.randn(4096, generator=g) * 1e-3,
                   torch.tensor([0.0, -0.0, 1.0, -1.0, 255.0, 256.0, 257.0, 258.0, 0.5, 1e-30, 3e38])))
    assert torch.equal(J.rn_bf16(x.double()), x.to(torch.bfloat16).double())
    # ties go to even, from the float64 value itself: 1 + 2^-8 is a tie in bf16, and a value
    # just above it would be rounded DOWN to the tie by a float32 in between
    tie = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert J.rn_bf16(tie).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]
    assert J.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.75, 200.0, 0.0])).tolist() == [
        2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 1.0, 2.0 ** -133]
    b = torch.tensor([1.0, 3.0, 0.0078125], dtype=torch.bfloat16)
    nxt = (b.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal(J.ulp_bf16(b.double()), nxt.double() - b.double())
    assert J.trunc_bf16(torch.tensor([1.999, -1.999])).tolist() == [1.9921875, -1.9921875]


@pytest.mark.parametrize("recipe", RECIPES)
def test_accepts_the_rounded_f32_restatement(recipe):
    _, j64, j32, e32 = normal_ref(*recipe)
    st = J.assert_half_ulp(J.rn_bf16(j32.double()), j64, e32)
    print(recipe, st)
    assert st["share"] == 0.0 and st["used_margin"] <= 1.0


@pytest.mark.parametrize("recipe", RECIPES)
def test_rejects_truncated_outputs_the_old_bar_accepts(recipe):
    _, j64, j32, e32 = normal_ref(*recipe)
    got = J.trunc_bf16(j32.double())
    assert old_close(got, j64)
    share = rejected(got, j64, e32)
    print(recipe, "truncation rejected on", share)
    assert share > 0.1


@pytest.mark.parametrize("c,shape", [(8, (5, 12, 33)), (16, (6, 9, 40))])
@pytest.mark.parametrize("round_a", [True, False])
def test_rejects_the_other_pair_rounding_the_old_bar_accepts(c, shape, round_a):
    """A pair sum rounded the way the OTHER kernel rounds it fails; its own way passes."""
    args, a64, b64, e32 = pair_ref(c, shape)
    want, alts = J.pair_wants(a64, b64, e32, round_a)
    assert torch.equal(want, J.pair_judge(*args, round_a))
    own = J.rn_bf16(J.pair_judge(*args, round_a, dtype=torch.float32).double())
    other = J.rn_bf16(J.pair_judge(*args, not round_a, dtype=torch.float32).double())
    assert J.assert_half_ulp(own, want, e32, alts)["share"] == 0.0
    assert old_close(other, want)
    share = rejected(other, want, e32, alts)
    print(c, shape, round_a, "other rounding rejected on", share)
    assert share > 1e-3


def test_rejects_a_third_pair_rounding():
    """Both terms rounded before the sum (three roundings) fits neither path."""
    args, a64, b64, e32 = pair_ref(8, (5, 12, 33))
    a32, b32 = J.pair_terms(*args, dtype=torch.float32)
    got = J.rn_bf16(J.rn_bf16(a32.double()) + J.rn_bf16(b32.double()))
    for round_a in (True, False):
        want, alts = J.pair_wants(a64, b64, e32, round_a)
        assert old_close(got, want)
        assert rejected(got, want, e32, alts) > 1e-3


def test_rejects_a_dropped_weight_a_dropped_column_and_a_bf16_partial_sum():
    b, cin, cout, k, shape = K128
    c, j64, j32, e32 = normal_ref(*K128)
    assert J.assert_half_ulp(J.rn_bf16(j32.double()), j64, e32)["share"] == 0.0

    def f32(x, w):
        return J.rn_bf16(J.conv_judge(x, w, c["scale"], c["shift"], True, k=k, dtype=torch.float32).double())
    w3 = c["w"].clone()
    w3[:, 77, 2, 0, 1] = 0  # mutant 3: one input channel's weight at one tap
    assert rejected(f32(c["x"], w3), j64, e32) > 0.01
    x4 = c["x"].clone()
    x4[..., -1] = 0  # mutant 4: the last W column not read
    assert rejected(f32(x4, c["w"]), j64, e32) > 0.01
    # mutant 5: the partial sum rounded to bf16 between two K chunks
    half = cin // 2
    p0 = J.rn_bf16(J.conv_raw(c["x"][:, :half], c["w"][:, :half], k, torch.float32).double()).float()
    raw = p0 + J.conv_raw(c["x"][:, half:], c["w"][:, half:], k, torch.float32)
    got5 = J.rn_bf16(J.epilogue(raw, c["scale"], c["shift"], True).double())
    assert old_close(got5, j64)
    assert rejected(got5, j64, e32) > 0.01


def test_relu_demands_an_exact_zero():
    want = torch.tensor([-1e-3, 0.5, 0.0])
    J.assert_half_ulp(torch.tensor([0.0, 0.5, 0.0]), want.clamp_min(0).double(), 1e-7)
    with pytest.raises(AssertionError):
        J.assert_half_ulp(torch.tensor([2.0 ** -20, 0.5, 0.0]), want.clamp_min(0).double(), 1e-8)


def test_integer_case_is_exact_at_the_largest_k_and_sees_the_mutants():
    b, cin, cout, k, shape = K128
    c = J.integer_case(0, cin, cout, k, shape, b)  # asserts its own condition
    raw = J.conv_raw(c["x"], c["w"], k)
    # float32 sums of these operands are the float64 ones, in torch's order as in any other
    assert torch.equal(J.conv_raw(c["x"], c["w"], k, torch.float32).double(), raw)
    for relu, r in ((True, None), (True, c["r"]), (False, c["r"])):
        want = J.epilogue(raw, c["scale"], c["shift"], relu, r)
        assert torch.equal(J.rn_bf16(want), want) and float(want.abs().max()) <= 256
        w3 = c["w"].clone()
        ci, tap = next((ci, tap) for ci in range(cin) for tap in range(27) if bool(w3[:, ci].reshape(cout, 27)[:, tap].any()))
        w3.view(cout, cin, 27)[:, ci, tap] = 0
        assert not torch.equal(J.conv_judge(c["x"], w3, c["scale"], c["shift"], relu, r, k=k), want)
        x4 = c["x"].clone()
        x4[..., -1] = 0
        assert not torch.equal(J.conv_judge(x4, c["w"], c["scale"], c["shift"], relu, r, k=k), want)


def test_integer_case_refuses_inexact_values():
    with pytest.raises(AssertionError):
        J.assert_bf16_exact(torch.tensor([257.0]))
    with pytest.raises(AssertionError):
        # 301 / 2 + 1 = 151.5: the spacing is 1 above 128
        J.assert_integer_exact(torch.tensor([301.0]).view(1, 1, 1, 1, 1).double(), torch.tensor([0.5]),
                               torch.tensor([1.0]), torch.zeros(1, 1, 1, 1, 1))


def test_integer_pair_and_costvolume_cases_hold_their_condition():
    p = J.integer_pair_case(3, 16, (4, 4, 16))
    want = J.pair_judge(p["xa"], p["wa"], p["xb"], p["wb"], p["sc"], p["sh"], True)
    assert torch.equal(want, J.pair_judge(p["xa"], p["wa"], p["xb"], p["wb"], p["sc"], p["sh"], False))
    J.integer_costvolume_case(1, 16, 16, 27, (5, 19))


def test_costvolume_judge_is_the_shifted_volume():
    g = torch.Generator().manual_seed(2)
    fl, fr = torch.randn(1, 2, 3, 7, generator=g), torch.randn(1, 2, 3, 7, generator=g)
    vol = J.build_cost_volume(fl, fr, 15)
    assert vol.shape == (1, 4, 5, 3, 7)
    for d in range(5):
        for w in range(7):
            want = torch.cat((fl[0, :, :, w], fr[0, :, :, w - d])).double() if w >= d else torch.zeros(4, 3).double()
            assert torch.equal(vol[0, :, d, :, w], want)


def test_pair_table():
    assert [[J.pair_rounds_a(c, s) for s in range(4)] for c in (8, 16)] == [
        [False, True, True, True], [False, True, True, False]]
