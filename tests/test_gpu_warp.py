"""``lea_forward_warp_f32`` on the device against the float32 judge of tests/warp_judge.py.

The bar is equality bit for bit of all four outputs, NaN pattern included, with no pixel left
out: every arithmetic step of the contract is one specified float32 operation, so a mismatch is
a contracted operation or a misread rule, never rounding.  Every output is written into a buffer
filled with a sentinel, with guard bands on both sides that must come back untouched.

Every sweep case's field is asserted to leave at least 0.5 % holes and 0.5 % occluded sources
in each item warped at a non-zero scale.  Widths 1 and 2 cannot hold two surfaces more than a
column apart: there the non-zero scales push everything out of view (all holes) and the
occlusion half of the requirement does not apply.
"""
import functools
import random

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels, synthesis
from tests import warp_judge as wj
from tests.golden_util import golden, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENT, SENT_BYTE, GUARD = 0x7FC0DEAD, 0xAB, 256
OUTS = ("warped", "zview", "state", "source")
INVALID = _lib.LEA_E_INVALID
SCALES3 = (0.0, -0.3, 1.3)  # one call: the identity, a negative scale, one above 1

# (H, W): the issue's widths, 300 and 1025 above the wave-row threshold of 256 and the
# workgroup's 256 lanes (a lane then owns a run of 2 and of 5 targets in the fill), the limit with
# H = 1; heights 1 .. 9, all but the first three with more rows (B * H) than the four of a
# wave-row workgroup
SWEEP = [(1, 1), (2, 2), (3, 3), (4, 63), (5, 64), (6, 65), (7, 67), (9, 131), (3, 257), (5, 300), (2, 1025),
         (1, kernels.FORWARD_WARP_MAX_W)]
IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_raw(image, disp, scales, exclude=None, max_diff=1.0, max_stretch=4.0, fill=1, fill_value=0.0, want=OUTS,
            pad=0):
    """The C entry, the wanted outputs in sentinel-filled buffers with guard bands: a dict of
    numpy arrays.  ``pad`` > 0 puts that many floats between the batch items of image and disp
    (batch strides above the block size)."""
    B, C, H, W = image.shape
    n = B * H * W
    if pad:
        im = np.full((B, C * H * W + pad), np.nan, F)
        im[:, :C * H * W] = image.reshape(B, -1)
        di = np.full((B, H * W + pad), np.nan, F)
        di[:, :H * W] = disp.reshape(B, -1)
    else:
        im, di = image, disp
    d_im, d_di, d_sc, d_ex = _dev(im), _dev(di), _dev(np.asarray(scales, F)), _dev(exclude)
    sizes = dict(warped=(n * C, torch.int32), zview=(n, torch.int32), state=(n, torch.uint8), source=(n, torch.int32))
    bufs = {k: torch.full((sizes[k][0] + 2 * GUARD,), SENT if sizes[k][1] == torch.int32 else SENT_BYTE, device=DEV,
                          dtype=sizes[k][1]) for k in want}
    p = {k: (bufs[k].data_ptr() + GUARD * bufs[k].element_size()) if k in bufs else None for k in OUTS}
    kernels.check(_lib.load().lea_forward_warp_f32(
        d_im.data_ptr(), C * H * W + pad, d_di.data_ptr(), H * W + pad, None if d_ex is None else d_ex.data_ptr(),
        d_sc.data_ptr(), B, C, H, W, max_diff, max_stretch, fill, fill_value, p["warped"], p["zview"], p["state"],
        p["source"], None), "lea_forward_warp_f32")
    torch.cuda.synchronize()
    out = {}
    for k, v in bufs.items():
        a = v.cpu().numpy()
        s = SENT if a.dtype == np.int32 else SENT_BYTE
        assert (a[:GUARD] == s).all() and (a[-GUARD:] == s).all(), f"{k}: a guard band was written"
        a = a[GUARD:-GUARD]
        assert not (a == s).any(), f"{k}: {int((a == s).sum())} elements were not written"
        out[k] = (a.view(F) if a.dtype == np.int32 else a).reshape((B, C, H, W) if k == "warped" else (B, H, W))
    assert wj.same_bits(d_im.cpu().numpy(), im) and wj.same_bits(d_di.cpu().numpy(), di)  # the inputs too
    return out


def assert_is_judge(out, j, what):
    for k in out:
        assert wj.same_bits(out[k], j[k]), (what, k, int((out[k].view(np.uint8) != j[k].view(np.uint8)).sum()))


def planted(disp, seed):
    """NaN, +-inf, +-1e30 and -0.0 in a copy of the field, where it is wide enough to keep a scene"""
    d = disp.copy()
    B, H, W = d.shape
    if W >= 63:
        rng = np.random.default_rng(seed)
        for v in (np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 1e-42):
            d[rng.integers(B), rng.integers(H), rng.integers(W)] = v
    return d


@functools.lru_cache(None)
def sweep_case(H, W, C=3):
    """(image, disp, exclude) of a sweep shape, B = 3, with the fractions asserted on the judge"""
    B = 3
    if W >= 63:
        disp = planted(wj.scene_field(B, H, W, max(12, W // 6), seed=H * 10007 + W), seed=W)
    elif W == 3:  # two surfaces by hand: item 1 at -0.3 hides x = 2 behind x = 0, item 2 at 1.3 x = 0 behind x = 2
        disp = np.stack([np.full((H, W), 0.25, F), np.tile(F([7, 0, 0]), (H, 1)), np.tile(F([0, 0, 1.6]), (H, 1))])
    else:  # one or two columns: out of view at the non-zero scales, so all holes
        disp = np.full((B, H, W), 9, F)
    img = wj.texture(B, C, H, W, seed=W + C)
    excl = (np.random.default_rng(W).uniform(size=(B, H, W)) < 0.02).astype(np.uint8) if W >= 63 else None
    j = wj.forward_warp_judge(img, disp, SCALES3, excl, fill=0)
    for b in (1, 2):
        one = {k: v[b:b + 1] for k, v in j.items()}
        holes, occ = wj.hole_fraction(one), wj.occluded_fraction(one, disp[b:b + 1], SCALES3[b:b + 1])
        assert holes >= 0.005, (H, W, b, holes)
        assert occ >= 0.005 or W < 3, (H, W, b, occ)
    return img, disp, excl


@functools.lru_cache(None)
def sweep_judge(H, W, fill, C=3):
    img, disp, excl = sweep_case(H, W, C)
    return wj.forward_warp_judge(img, disp, SCALES3, excl, fill=fill, fill_value=-2.5)


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("shape", SWEEP, **IDS)
def test_sweep_is_the_judge_bit_for_bit(shape, fill):
    img, disp, excl = sweep_case(*shape)
    out = run_raw(img, disp, SCALES3, excl, fill=fill, fill_value=-2.5)
    assert_is_judge(out, sweep_judge(*shape, fill), (shape, fill))


@pytest.mark.parametrize("C", [1, 4])
def test_one_and_four_channels(C):
    img, disp, excl = sweep_case(7, 67, C)
    assert_is_judge(run_raw(img, disp, SCALES3, excl, fill_value=-2.5), sweep_judge(7, 67, 1, C), C)


@pytest.mark.parametrize("shape", [(4, 63), (5, 300)], **IDS)
def test_each_output_in_turn_null_and_alone(shape):
    img, disp, excl = sweep_case(*shape)
    for fill in (0, 1):
        j = sweep_judge(*shape, fill)
        for k in OUTS:
            assert_is_judge(run_raw(img, disp, SCALES3, excl, fill=fill, fill_value=-2.5,
                                    want=tuple(o for o in OUTS if o != k)), j, ("without", k))
            assert_is_judge(run_raw(img, disp, SCALES3, excl, fill=fill, fill_value=-2.5, want=(k,)), j, ("only", k))


def test_batch_strides_above_the_block():
    img, disp, excl = sweep_case(7, 67)
    assert_is_judge(run_raw(img, disp, SCALES3, excl, fill_value=-2.5, pad=37), sweep_judge(7, 67, 1), "strided")


def test_excluded_and_non_finite_items_are_holes():
    H, W = 5, 131
    img, disp = wj.texture(3, 3, H, W), wj.scene_field(3, H, W, 20, seed=3)
    excl = np.zeros((3, H, W), np.uint8)
    excl[0] = 1            # every pixel excluded
    excl[1, :, ::2] = 200  # any non-zero byte; isolated pixels come through the point rule
    excl[2, 2] = 1         # a row with no hit between rows that have some
    for fill in (0, 1):
        out = run_raw(img, disp, [1.0, 0.0, 0.7], excl, fill=fill, fill_value=4.0)
        assert_is_judge(out, wj.forward_warp_judge(img, disp, [1.0, 0.0, 0.7], excl, fill=fill, fill_value=4.0), fill)
        assert out["state"][0].all() and (out["warped"][0] == 4.0).all() and np.isnan(out["zview"][0]).all()
        assert out["state"][2, 2].all() and (out["warped"][2, :, 2] == 4.0).all()
        assert np.array_equal(out["state"][1] == 0, excl[1] == 0)
    # a non-finite scale makes its item holes; the third item is untouched by its neighbours
    for scales in ([np.inf, np.nan, 1.0], [-np.inf, 1.0, np.nan]):
        out = run_raw(img, disp, scales, None, fill=1, fill_value=4.0)
        assert_is_judge(out, wj.forward_warp_judge(img, disp, scales, None, fill=1, fill_value=4.0), scales)
        for b, s in enumerate(scales):
            assert bool(out["state"][b].all()) == (not np.isfinite(s))


def test_any_disparity_and_scale_values_are_memory_safe():
    """NaN, infinities, +-1e30, denormals and random bits as disparities and scales: the guards
    hold and the outputs are the judge's"""
    H, W = 3, 300
    rng = np.random.default_rng(8)
    img = wj.texture(3, 2, H, W)
    special = F([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 1e-42, -1e-42, 3.4e38, 5.0, -5.0, 0.5, 299, -299, 1e7])
    disp = special[rng.integers(0, len(special), (3, H, W))]
    bits = rng.integers(0, 2 ** 32, (3, H, W), dtype=np.uint64).astype(np.uint32).view(F)
    for d, scales in ((disp, [1.0, -1e30, 1e-40]), (disp, [3e38, -1.0, 0.5]), (bits, [1.0, -2.0, 1e30]),
                      (wj.scene_field(3, H, W, 40, seed=2), [50.0, -50.0, 1e30])):  # out of view on both sides
        for md, ms in ((1.0, 4.0), (3.0e38, 64.0)):
            out = run_raw(img, d, scales, None, md, ms, 1, 0.0)
            assert_is_judge(out, wj.forward_warp_judge(img, d, scales, None, md, ms, 1, 0.0), (scales, md, ms))


def test_ties_on_every_target():
    """constant integer disparity at integer scales: a point and two segments meet on every
    target with the same z; the larger column wins, its segment over its point (a = 0)"""
    H, W = 2, 131
    img = wj.texture(3, 3, H, W)
    disp = np.stack([np.full((H, W), 4, F), np.full((H, W), -3, F), np.full((H, W), 0, F)])
    disp[2, :, ::3] = -0.0  # equal to +0 as a depth; a lerp's (1 * -0) + (0 * d) is +0, as the judge has it
    scales = [1.0, 2.0, -7.0]
    out = run_raw(img, disp, scales, None, fill=0, fill_value=-1.0, want=OUTS)
    assert_is_judge(out, wj.forward_warp_judge(img, disp, scales, None, fill=0, fill_value=-1.0), "ties")
    assert wj.same_bits(out["warped"][0, :, :, :W - 4], img[0, :, :, 4:])           # a shift by 4, exact
    assert wj.same_bits(out["warped"][1, :, :, 6:], img[1, :, :, :W - 6])           # by -6
    assert wj.same_bits(out["warped"][2], img[2]) and np.array_equal(out["zview"][2], disp[2])
    assert np.array_equal(out["source"][0, 0, :W - 4], np.arange(4, W, dtype=F))


def test_spans_at_and_just_past_the_thresholds():
    d, im = wj.threshold_rows()
    for s in wj.THRESHOLD_SCALES:
        for fill in (0, 1):
            out = run_raw(im, d, [s], None, 0.5, 2.0, fill, 9.0)
            assert_is_judge(out, wj.forward_warp_judge(im, d, [s], None, 0.5, 2.0, fill, 9.0), (s, fill))
    for extra, hole in ((F(0), 0), (F(2.0 ** -20), 1)):  # tests/test_warp_cpu.py: test_thresholds_by_hand
        d = np.full((1, 1, 16), 5, F)
        d[0, 0, 11:] = F(4) - extra
        out = run_raw(wj.texture(1, 1, 1, 16, seed=4), d, [1.0], None, 4.0, 2.0, 0, 0.0)
        assert out["state"][0, 0, 6] == hole


def raw_call(image, disp, excl, scales, B, C, H, W, md, ms, fill, warped, zview, state, source, ibs=None, dbs=None):
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()  # noqa: E731
    return _lib.load().lea_forward_warp_f32(
        ptr(image), C * H * W if ibs is None else ibs, ptr(disp), H * W if dbs is None else dbs, ptr(excl), ptr(scales),
        B, C, H, W, md, ms, fill, 0.0, ptr(warped), ptr(zview), ptr(state), ptr(source), None)


def test_refusals_through_the_raw_entry():
    """tests/asan/warp_asan.cpp on the device: every refusal is LEA_E_INVALID before any launch,
    names the entry, and writes nothing"""
    B, C, H, W = 2, 3, 4, 6
    n = B * H * W
    img, disp, sc = (torch.full((k,), -7.0, device=DEV) for k in (C * n, n, B))
    wa, zv, so = (torch.full((k,), -7.0, device=DEV) for k in (C * n, n, n))
    ex, st = (torch.full((n,), 9, device=DEV, dtype=torch.uint8) for _ in range(2))
    good = dict(image=img, disp=disp, excl=ex, scales=sc, B=B, C=C, H=H, W=W, md=1.0, ms=4.0, fill=1, warped=wa, zview=zv,
                state=st, source=so)
    bad = [dict(image=None), dict(disp=None), dict(scales=None), dict(warped=None, zview=None, state=None, source=None),
           dict(B=0), dict(H=-4), dict(W=0), dict(W=kernels.FORWARD_WARP_MAX_W + 1), dict(B=65536, H=65536),
           dict(C=0), dict(C=5), dict(ibs=C * H * W - 1), dict(ibs=-1), dict(dbs=H * W - 1), dict(dbs=0),
           dict(md=-0.5), dict(md=float("nan")), dict(md=float("inf")), dict(ms=0.5), dict(ms=64.5),
           dict(ms=float("nan")), dict(ms=float("inf")), dict(fill=2),
           dict(warped=img), dict(warped=img.data_ptr() + 4 * (C * n - 1)), dict(zview=disp), dict(zview=sc, B=1),
           dict(state=ex), dict(state=ex.data_ptr() + n - 1), dict(state=img), dict(source=zv),
           dict(source=zv.data_ptr() + 4 * (n - 1)), dict(zview=wa.data_ptr() + 4 * (C * n - 1)),
           dict(state=so), dict(state=zv.data_ptr() + 4 * n - 1),
           dict(warped=None, zview=None, source=None, state=ex)]
    lib = _lib.load()
    for kw in bad:
        assert raw_call(**dict(good, **kw)) == INVALID, kw
        assert b"lea_forward_warp_f32" in lib.lea_last_error(), kw
    torch.cuda.synchronize()
    for t in (img, disp, sc, wa, zv, so):
        assert (t == -7.0).all()
    assert (ex == 9).all() and (st == 9).all()
    assert raw_call(**good) == 0  # and the good call is one
    torch.cuda.synchronize()


def test_wrapper_checks_and_shapes():
    img, disp, excl = sweep_case(7, 67)
    di, dd = _dev(img), _dev(disp)
    v = kernels.forward_warp(di, dd, 0.5, _dev(excl), fill_value=-2.5, want_source=True)
    j = wj.forward_warp_judge(img, disp, [0.5] * 3, excl, fill_value=-2.5)
    assert_is_judge(dict(warped=v.image.cpu().numpy(), zview=v.zview.cpu().numpy(), state=v.state.cpu().numpy(),
                         source=v.source.cpu().numpy()), j, "wrapper")
    v = kernels.forward_warp(di, dd, _dev(F(SCALES3)), _dev(excl).bool(), want_zview=False, want_state=False)
    assert v.zview is None and v.state is None and v.source is None
    assert wj.same_bits(v.image.cpu().numpy(), wj.forward_warp_judge(img, disp, SCALES3, excl)["warped"])
    # a channel slice and a batch slice go in without a copy of the caller's making
    big = _dev(wj.texture(4, 4, 7, 67, seed=5))
    v = kernels.forward_warp(big[1:, :3], dd, 1.0)
    assert wj.same_bits(v.image.cpu().numpy(), wj.forward_warp_judge(big[1:, :3].cpu().numpy(), disp, [1.0] * 3)["warped"])
    for bad in (dict(image=di.double()), dict(image=di.cpu()), dict(disp=dd[:2]), dict(image=di[0]),
                dict(scale=torch.ones(2, device=DEV)), dict(scale=torch.ones(3)), dict(scale="1"),
                dict(exclude=torch.zeros(3, 7, 67, device=DEV)), dict(max_diff=-1), dict(max_diff=float("nan")),
                dict(max_stretch=0.5), dict(max_stretch=65), dict(fill_value=None),
                dict(image=torch.zeros(1, 5, 7, 67, device=DEV), disp=dd[:1]),
                dict(image=torch.zeros(1, 1, 1, kernels.FORWARD_WARP_MAX_W + 1, device=DEV),
                     disp=torch.zeros(1, 1, kernels.FORWARD_WARP_MAX_W + 1, device=DEV))):
        with pytest.raises((ValueError, _lib.HipKernelError)):
            kernels.forward_warp(**dict(dict(image=di, disp=dd), **bad))


def test_captured_call_replays_with_new_scales():
    img, disp, excl = sweep_case(9, 131)
    di, dd, de = _dev(img), _dev(disp), _dev(excl)
    sc = _dev(F([1.0, 0.5, -0.2]))
    call = lambda: kernels.forward_warp(di, dd, sc, de, fill_value=-2.5, want_source=True)  # noqa: E731
    a, b = call(), call()
    for x, y in zip(a, b):  # two calls, the same bits
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    graph.replay()
    for x, y in zip(out, a):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    sc.copy_(_dev(F(SCALES3)))  # in place: the replay reads them on the device
    graph.replay()
    torch.cuda.synchronize()
    got = dict(warped=out.image.cpu().numpy(), zview=out.zview.cpu().numpy(), state=out.state.cpu().numpy(),
               source=out.source.cpu().numpy())
    assert_is_judge(got, sweep_judge(9, 131, 1), "replay")
    assert not torch.equal(out.image, a.image)


def test_lr_check_agrees_on_the_layered_scene():
    """what exists already, the other way round: with the s = 1 view's zview as the right-view
    disparity, lea_disparity_lr_check finds consistent exactly the left pixels that won their target"""
    sc = wj.layered_scene()
    dl = _dev(sc["disp_left"])
    v = kernels.forward_warp(_dev(sc["left"]), dl, 1.0, fill=False, want_source=True)
    hit = (v.state == 0).cpu().numpy()[0]
    assert np.array_equal(hit, np.broadcast_to(sc["right_from_left"], hit.shape))
    assert wj.same_bits(v.image.cpu().numpy()[0][:, hit], sc["right"][0][:, hit])
    lr = kernels.lr_check(dl, v.zview.nan_to_num(nan=-1000.0), 0.5, want_filled=False)
    src = v.source.cpu().numpy()[0]
    H, W = hit.shape
    won = np.zeros((H, W), bool)
    for y in range(H):
        for u in range(W):
            if hit[y, u]:
                assert src[y, u] == int(src[y, u])  # integer disparities: every winner has a = 0
                won[y, int(src[y, u])] = True
    assert np.array_equal(lr.state.cpu().numpy()[0] == 0, won) and 0.5 < won.mean() < 1


@pytest.mark.parametrize("with_right", [True, False])
def test_augment_on_the_device(with_right):
    B, H, W = 4, 6, 131
    dl = wj.scene_field(B, H, W, 20, seed=11)
    dl[0, 0, :4], dl[1, 1, :4] = 0.0, 1000.0
    dr = wj.scene_field(B, H, W, 20, seed=12)
    left, right = wj.texture(B, 3, H, W, 1), wj.texture(B, 3, H, W, 2)
    rng = random.Random(3)
    draws = [synthesis.sample_warp_scale(0.5, 0.3, rng) for _ in range(B)]
    assert {c for c, _ in draws} == {True, False}
    aug = synthesis.DisparityScaleAugment(0.5, 0.3, rng=random.Random(3), maxdisp=192)
    out = aug(_dev(left), _dev(right), _dev(dl), _dev(dr) if with_right else None)
    scales = np.array([s for _, s in draws], F)
    assert np.array_equal(out.scales.cpu().numpy(), scales) and out.chosen.tolist() == [c for c, _ in draws]
    j = wj.forward_warp_judge(right, dr, scales - F(1)) if with_right else wj.forward_warp_judge(left, dl, scales)
    valid = (dl > 0.001) & (dl < 192)
    got_r, got_d, got_s = out.right.cpu().numpy(), out.disp_left.cpu().numpy(), out.state.cpu().numpy()
    for b, (c, s) in enumerate(draws):
        if c:
            assert wj.same_bits(got_r[b], j["warped"][b]) and np.array_equal(got_s[b], j["state"][b])
            assert wj.same_bits(got_d[b], np.where(valid[b], dl[b] * F(s), dl[b]))
        else:
            assert wj.same_bits(got_r[b], right[b]) and wj.same_bits(got_d[b], dl[b]) and not got_s[b].any()


def test_view_scene_and_predict_cli(tmp_path):
    """A 120 x 300 sceneflow-layout pair through a 96 x 192 crop: --novel_view adds the two files
    and moves nothing else; they are the wrapper's output on the written map."""
    from PIL import Image
    from leastereo_amd import predict as P
    g = golden("c1_sceneflow")
    for side in ("left", "right"):
        d = tmp_path / "frames_finalpass" / "S" / side
        d.mkdir(parents=True)
        Image.fromarray(g[side + "_u8"][:120, :300]).save(d / "0001.png")
    (tmp_path / "list.txt").write_text("S/left/0001.png\n")
    torch.save({"state_dict": {"module." + k: v for k, v in state_dict().items()}}, tmp_path / "ckpt.pth")
    base = ["--sceneflow=1", "--maxdisp=48", "--crop_height=96", "--crop_width=192", f"--data_path={tmp_path}/",
            f"--test_list={tmp_path}/list.txt", f"--resume={tmp_path}/ckpt.pth"]
    assert P.main(base + [f"--save_path={tmp_path}/plain/"]) == 0
    assert P.main(base + [f"--save_path={tmp_path}/view/", "--novel_view=1", "--view_fill=0"]) == 0
    assert sorted(p.name for p in (tmp_path / "view").iterdir()) == sorted(
        [p.name for p in (tmp_path / "plain").iterdir()] + ["0_view.png", "0_view_holes.png"])
    disp = np.load(tmp_path / "view" / "0.npy")
    assert np.array_equal(disp, np.load(tmp_path / "plain" / "0.npy")) and disp.shape == (96, 192)
    view = np.asarray(Image.open(tmp_path / "view" / "0_view.png"))
    holes = np.asarray(Image.open(tmp_path / "view" / "0_view_holes.png"))
    assert view.shape == (96, 192, 3) and holes.shape == (96, 192)
    x0, y0 = P.map_origin(120, 300, 96, 192)
    crop = g["left_u8"][:120, :300][y0:y0 + 96, x0:x0 + 192, :3]
    img = _dev(crop).permute(2, 0, 1).float().contiguous()[None]
    want = kernels.forward_warp(img, _dev(disp)[None], 1.0, fill=False)
    assert np.array_equal(view, want.image[0].round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy())
    assert np.array_equal(holes != 0, (want.state[0] != 0).cpu().numpy())
    # the scene path's helper gives the same view of the same map
    from leastereo_amd import scene
    res = scene.SceneResult(disp=_dev(disp))
    v = scene.view_scene(res, crop, 1.0, use="disp", fill=False)
    assert torch.equal(v.image, want.image[0]) and torch.equal(v.state, want.state[0])
    with pytest.raises(ValueError):
        scene.view_scene(res, crop, 1.0, use="filled")
    with pytest.raises(ValueError):
        scene.view_scene(res, crop, 1.0, use="nothing")
