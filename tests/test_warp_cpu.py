"""The host side of the view synthesis, without a device: the two forms of the judge of
tests/warp_judge.py against each other, the scale-0 identity, a layered scene whose right view is
known by construction, the reference's draws, ``DisparityScaleAugment``'s host logic with the
judge standing in for the kernel, the predict.py flags and the wiring of the sanitizer driver."""
import os
import random
import subprocess

import numpy as np
import pytest
import torch

from leastereo_amd import kernels, synthesis
from tests import warp_judge as wj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FIELDS = [(5, 67, 12), (9, 131, 24), (3, 257, 40)]  # H, W, dmax
SCALES = [1.0, -0.3, 0.3, 1.3, 0.5]
OUTS = ("warped", "zview", "state", "source")


def assert_same(a, b, what):
    for k in OUTS:
        assert wj.same_bits(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("field", FIELDS, ids=lambda f: "x".join(map(str, f)))
def test_fields_have_holes_and_occlusions(field):
    """what every GPU case is asked to show, on the issue's three fields and five scales"""
    H, W, dmax = field
    disp = wj.scene_field(1, H, W, dmax, seed=W)
    img = wj.texture(1, 1, H, W)
    for s in SCALES:
        j = wj.forward_warp_judge(img, disp, [s], fill=0)
        holes, occ = wj.hole_fraction(j), wj.occluded_fraction(j, disp, [s])
        assert holes >= 0.005 and occ >= 0.005, (field, s, holes, occ)
        assert holes <= 0.3 and occ <= 0.3, (field, s, holes, occ)


@pytest.mark.parametrize("fill", [0, 1])
def test_the_two_judge_forms_agree(fill):
    H, W, dmax = 3, 67, 12
    disp = wj.scene_field(3, H, W, dmax, seed=5)
    disp[0, 0, 5], disp[1, 1, 9], disp[2, 2, 30], disp[0, 1, 40] = np.nan, np.inf, -1e30, -0.0
    disp[2, 1] = 4.0  # constant integer disparity: ties on every target at an integer scale
    disp[1, 2] = np.nan  # a row with no hit
    img = wj.texture(3, 2, H, W)
    excl = (np.random.default_rng(2).uniform(size=(3, H, W)) < 0.05).astype(np.uint8)
    for scales in ([1.0, -0.3, 1.3], [0.0, 0.5, 2.0], [np.inf, 1.0, -1.0]):
        a = wj.forward_warp_judge(img, disp, scales, excl, 1.0, 4.0, fill, -3.0, form="scatter")
        b = wj.forward_warp_judge(img, disp, scales, excl, 1.0, 4.0, fill, -3.0, form="gather")
        assert_same(a, b, scales)
    # thresholds exactly at and just past max_diff and max_stretch (the hand cases of the GPU test)
    d, im = wj.threshold_rows()
    for s in wj.THRESHOLD_SCALES:
        a = wj.forward_warp_judge(im, d, [s], None, 0.5, 2.0, fill, 9.0, form="scatter")
        b = wj.forward_warp_judge(im, d, [s], None, 0.5, 2.0, fill, 9.0, form="gather")
        assert_same(a, b, ("thresholds", s))


def test_thresholds_by_hand():
    """den = 2 = max_stretch is a segment covering three targets, the next float above is none"""
    for extra, expect in ((F(0), 0), (F(2.0 ** -20), 1)):
        # d0 = 5 up to x = 10, d1 = 4 - extra from x = 11: t = 5 and 7 + extra, both exact, den = 2 + extra
        d = np.full((1, 1, 16), 5, F)
        d[0, 0, 11:] = F(4) - extra
        im = wj.texture(1, 1, 1, 16, seed=4)
        j = wj.forward_warp_judge(im, d, [1.0], None, 4.0, 2.0, 0, 0.0)
        # x = 10 lands on 5, x = 11 on 7 (+ extra): target 6 is covered only by the segment
        assert j["state"][0, 0, 6] == expect, (extra, j["state"][0, 0])
        if not expect:
            assert j["source"][0, 0, 6] == F(10.5) and j["zview"][0, 0, 6] == F(4.5)


def test_scale_zero_is_the_identity_bit_for_bit():
    H, W = 4, 67
    disp = wj.scene_field(2, H, W, 12, seed=7)
    img = wj.texture(2, 3, H, W)
    for form in ("scatter", "gather"):
        j = wj.forward_warp_judge(img, disp, [0.0, -0.0], form=form)
        assert wj.same_bits(j["warped"], img) and wj.same_bits(j["zview"], disp)
        assert not j["state"].any()
        assert np.array_equal(j["source"], np.broadcast_to(np.arange(W, dtype=F), (2, H, W)))
    # isolated pixels (both neighbours excluded or not finite) come through the point rule
    excl = np.zeros((2, H, W), np.uint8)
    excl[:, :, 0::2] = 1
    disp[0, 0, 3] = np.nan
    j = wj.forward_warp_judge(img, disp, [0.0, 0.0], excl, fill=0, fill_value=-5.0)
    keep = (excl == 0) & np.isfinite(disp)
    assert np.array_equal(j["state"] == 0, keep)
    for c in range(3):
        assert wj.same_bits(j["warped"][:, c][keep], img[:, c][keep])
        assert (j["warped"][:, c][~keep] == -5.0).all()
    assert wj.same_bits(j["zview"][keep], disp[keep]) and np.isnan(j["zview"][~keep]).all()


def test_layered_scene_holds_its_ground_truth():
    sc = wj.layered_scene()
    for form in ("scatter", "gather"):
        j = wj.forward_warp_judge(sc["left"], sc["disp_left"], [1.0], fill=0, form=form)
        hit = j["state"][0] == 0
        assert np.array_equal(hit, np.broadcast_to(sc["right_from_left"], hit.shape))
        assert 0.02 < 1 - hit.mean() < 0.5
        for c in range(3):
            assert wj.same_bits(j["warped"][0, c][hit], sc["right"][0, c][hit])
        assert wj.same_bits(j["zview"][0][hit], sc["disp_right"][0][hit])
    # and back: the right view at s = 0 of view_from_right's scale (s - 1 = -1) is the left view
    j = wj.forward_warp_judge(sc["right"], sc["disp_right"], [-1.0], fill=0)
    hit = j["state"][0] == 0
    assert hit.mean() > 0.5
    for c in range(3):
        assert wj.same_bits(j["warped"][0, c][hit], sc["left"][0, c][hit])
    assert wj.same_bits(j["zview"][0][hit], sc["disp_left"][0][hit])
    # filled holes take the background side
    j = wj.forward_warp_judge(sc["left"], sc["disp_left"], [1.0], fill=1)
    holes = j["state"][0] != 0
    assert (j["zview"][0][holes] == 3).all()  # the background layer's disparity


def reference_draws(prob, max_scale_diff):
    """warp_aug's two draws, restated literally: choose([1 - p, p]) walks the cumulative sums."""
    rnd = random.random()
    c, prob_sum = 0, 0
    for p in [1 - prob, prob]:
        prob_sum += p
        if rnd < prob_sum:
            break
        c += 1
    if c == 0:
        return False, 1.0
    return True, 1 + (2 * random.random() - 1) * max_scale_diff


@pytest.mark.parametrize("prob", [0, 0.5, 1])
def test_sample_warp_scale_makes_the_reference_draws(prob):
    random.seed(1234)
    want = [reference_draws(prob, 0.3) for _ in range(50)]
    after = random.random()
    random.seed(1234)
    got = [synthesis.sample_warp_scale(prob, 0.3) for _ in range(50)]
    assert got == want and random.random() == after  # the same values from the same number of draws
    assert all(c for c, _ in got) if prob == 1 else True
    assert not any(c for c, _ in got) if prob == 0 else True
    if prob == 0.5:
        assert 10 < sum(c for c, _ in got) < 40
        assert all(0.7 <= s <= 1.3 for _, s in got)
    rng = random.Random(7)
    a = [synthesis.sample_warp_scale(prob, 0.2, rng) for _ in range(5)]
    rng = random.Random(7)
    assert a == [synthesis.sample_warp_scale(prob, 0.2, rng) for _ in range(5)]


def judge_as_kernel(image, disp, scale=1.0, exclude=None, max_diff=1.0, max_stretch=4.0, fill=True, fill_value=0.0,
                    want_zview=True, want_state=True, want_source=False):
    b = image.shape[0]
    sc = scale.numpy() if isinstance(scale, torch.Tensor) else np.full(b, scale, F)
    j = wj.forward_warp_judge(image.numpy(), disp.numpy(), sc, None if exclude is None else exclude.numpy(),
                              max_diff, max_stretch, int(fill), fill_value)
    return kernels.WarpedView(torch.from_numpy(j["warped"]), torch.from_numpy(j["zview"]) if want_zview else None,
                              torch.from_numpy(j["state"]) if want_state else None,
                              torch.from_numpy(j["source"]) if want_source else None)


@pytest.mark.parametrize("with_right", [True, False])
def test_augment_host_logic_with_the_judge_as_the_kernel(monkeypatch, with_right):
    monkeypatch.setattr(kernels, "forward_warp", judge_as_kernel)
    B, H, W = 4, 3, 67
    dl = wj.scene_field(B, H, W, 12, seed=11)
    dl[0, 0, :4], dl[1, 1, :4] = 0.0, 1000.0  # invalid targets: no value, and the transform's pad
    dr = wj.scene_field(B, H, W, 12, seed=12)
    left, right = wj.texture(B, 3, H, W, 1), wj.texture(B, 3, H, W, 2)
    rng = random.Random(3)
    draws = [synthesis.sample_warp_scale(0.5, 0.3, rng) for _ in range(B)]
    assert {c for c, _ in draws} == {True, False}  # this seed mixes both
    aug = synthesis.DisparityScaleAugment(0.5, 0.3, rng=random.Random(3), device="cpu", maxdisp=192)
    t = torch.from_numpy
    out = aug(t(left), t(right), t(dl), t(dr) if with_right else None)
    scales = np.array([s for _, s in draws], F)
    assert np.array_equal(out.scales.numpy(), scales)
    assert out.chosen.tolist() == [c for c, _ in draws]
    assert out.left.data_ptr() == t(left).data_ptr() or np.array_equal(out.left.numpy(), left)
    if with_right:
        j = wj.forward_warp_judge(right, dr, scales - F(1))
    else:
        j = wj.forward_warp_judge(left, dl, scales)
    valid = (dl > 0.001) & (dl < 192)
    for b, (c, s) in enumerate(draws):
        if c:
            assert wj.same_bits(out.right[b].numpy(), j["warped"][b])
            assert np.array_equal(out.state[b].numpy(), j["state"][b])
            want = np.where(valid[b], dl[b] * F(s), dl[b])
            assert wj.same_bits(out.disp_left[b].numpy(), want)
            assert not np.array_equal(out.right[b].numpy(), right[b])
        else:
            assert wj.same_bits(out.right[b].numpy(), right[b])
            assert wj.same_bits(out.disp_left[b].numpy(), dl[b])
            assert not out.state[b].any()
    assert out.disp_left[0, 0, 0] == 0.0 and out.disp_left[1, 1, 0] == 1000.0


def test_augment_refuses_bad_arguments():
    with pytest.raises(ValueError):
        synthesis.DisparityScaleAugment(prob=1.5)
    with pytest.raises(ValueError):
        synthesis.DisparityScaleAugment(max_scale_diff=-0.1)
    aug = synthesis.DisparityScaleAugment(device="cpu")
    with pytest.raises(ValueError):
        aug(torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 6))


def test_predict_flags():
    from leastereo_amd import predict
    from leastereo_amd.config import obtain_predict_args
    base = ["--crop_height=96", "--crop_width=192", "--data_path=d/", "--test_list=l.txt"]
    assert predict.novel_view_options(obtain_predict_args(base)) is None
    assert predict.novel_view_options(obtain_predict_args(base + ["--view_fill=0"])) is None  # off: nothing is looked at
    assert predict.novel_view_options(obtain_predict_args(base + ["--novel_view=0.5"])) == dict(s=0.5, fill=True)
    assert predict.novel_view_options(obtain_predict_args(base + ["--novel_view=-0.25", "--view_fill=0"])) == dict(
        s=-0.25, fill=False)
    assert predict.novel_view_options(obtain_predict_args(base + ["--novel_view=0"])) == dict(s=0.0, fill=True)
    for bad in ("nan", "inf", "-inf"):
        with pytest.raises(ValueError, match="--novel_view"):
            predict.novel_view_options(obtain_predict_args(base + [f"--novel_view={bad}"]))
    with pytest.raises(SystemExit):
        obtain_predict_args(base + ["--novel_view=1", "--view_fill=2"])
    with pytest.raises(NotImplementedError, match="--novel_view"):
        predict.novel_view_options(obtain_predict_args(base + ["--novel_view=1", "--satellite=1"]))
    # main refuses before it needs a device
    with pytest.raises(ValueError, match="--novel_view"):
        predict.main(base + ["--sceneflow=1", "--novel_view=nan"])
    # a map wider than the kernel's limit is refused with the limit in the message, before any device work
    wide = np.zeros((2, kernels.FORWARD_WARP_MAX_W + 1), F)
    with pytest.raises(ValueError, match=str(kernels.FORWARD_WARP_MAX_W)):
        predict.novel_view_of_map(wide, None, np.zeros(wide.shape + (3,), np.uint8), 1.0)


def test_header_limit_and_wrapper_limit_agree():
    src = open(os.path.join(REPO, "include", "leastereo_hip.h")).read()
    assert f"#define LEA_FORWARD_WARP_MAX_W {kernels.FORWARD_WARP_MAX_W}\n" in src
    assert kernels.FORWARD_WARP_MAX_W >= 4096


def test_asan_driver_is_wired_into_make_asan():
    """`make asan` links the driver with every unit and runs it: asked of make itself (a dry run
    of the whole target), so the run is tests/test_asan_cpu.py's."""
    assert os.path.isfile(os.path.join(REPO, "tests", "asan", "warp_asan.cpp"))
    plan = subprocess.run(["make", "-n", "-B", "asan"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert plan.returncode == 0, plan.stderr
    link = [l for l in plan.stdout.splitlines() if " -o build/asan/warp_asan " in l]
    assert len(link) == 1 and "build/asan/warp_asan_main.o" in link[0] and "build/asan/forward_warp.o" in link[0]
    assert "ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/warp_asan" in plan.stdout.splitlines()
