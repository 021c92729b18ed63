"""The speckle filter on the GPU (lea_disparity_speckle_f32, kernels.speckle_filter,
LEAStereo.forward_refined(speckle=...) / graphed(refine=dict(speckle=...)), scene.speckle_scene,
scene.refine_scene(speckle=...)).

Every case compares labels, size, state and filtered with tests/speckle_judge.py bit for bit,
no pixel left out: the outputs are integers (and copies of the input's floats), so there is no
tolerance anywhere.  The kernel's tile is 64 x 16: the shapes straddle it at least twice in
both axes ((2, 67, 131), (1, 130, 70), and (1, 33, 129) = 2 tiles + 1 exactly) and stay below
40 k pixels.

The random cases assert, on the judge, at least 50 components on each side of max_size, so that
none can pass by removing nothing or everything.  That condition is checked where it can hold:
at max_diff 0.5 and 1.0 on the fields of 4000 pixels and more.  A 1 x 257 line holds at most
12 components above 20 px, a single pixel one component, and at max_diff 0 the recipe's noise
leaves singletons only; those cases still compare every pixel with the judge.
"""
import functools

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels, scene
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from tests import speckle_judge as sj
from tests.golden_util import golden, normal, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("labels", "size", "state", "filtered")
RANDOM_SHAPES = [(1, 1, 1), (1, 1, 257), (1, 33, 1), (2, 67, 131), (1, 130, 70), (1, 33, 129)]
IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)  # a copy: the references are read-only


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_is_judge(out, want, what=""):
    for name in FIELDS:
        got = getattr(out, name)
        assert got is not None, name
        g, w = _bits(got), _bits(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = int((g != w).sum())
        assert bad == 0, f"{what} {name}: {bad} of {g.size} pixels differ, first at {np.argwhere(g != w)[0]}"


def check(disp, exclude, max_diff, max_size, fill=0.0, what=""):
    out = kernels.speckle_filter(_dev(disp), _dev(exclude), max_size, max_diff, fill, want_labels=True)
    want = sj.judge(disp, exclude, max_diff, max_size, fill)
    assert_is_judge(out, want, what)
    return out, want


@functools.lru_cache(maxsize=None)
def random_case(shape):
    d, e = sj.random_field(shape, seed=sum(shape))
    d.setflags(write=False), e.setflags(write=False)
    return d, e


# ------------------------------------------------------------------ random fields
@pytest.mark.parametrize("max_diff", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, **IDS)
def test_random_fields(shape, max_diff):
    d, e = random_case(shape)
    out, want = check(d, e, max_diff, 20, what=f"{shape} max_diff {max_diff}")
    n = sj.component_sizes(want["labels"], want["size"])
    small, large = int((n <= 20).sum()), int((n > 20).sum())
    removed = float(((want["state"] == 3) & (want["labels"] >= 0)).sum()) / max(int((want["labels"] >= 0).sum()), 1)
    print(f"{shape} max_diff {max_diff}: {n.size} components, {small} of at most 20 px, {large} larger, "
          f"{100 * removed:.1f} % of the non-wall pixels removed")
    if shape[1] * shape[2] >= 4000 and max_diff > 0:
        assert small >= 50 and large >= 50


def test_random_field_without_exclude_and_2d():
    d, _ = random_case((1, 130, 70))
    out, _ = check(d[0], None, 1.0, 20)
    assert out.state.shape == (130, 70)


# ------------------------------------------------------------------ structures
def test_serpentine():
    _, want = check(sj.serpentine(), None, 1.0, 200)
    assert want["size"][0, 0] == 1820 and (want["state"][0] == 0).all()   # crosses every tile border
    check(sj.serpentine(), None, 1.0, 1820)
    check(sj.serpentine().T.copy(), None, 1.0, 200)                       # and the column-wise one


def test_spiral():
    _, want = check(sj.spiral(), None, 1.0, 200)
    assert sj.component_sizes(want["labels"], want["size"]).size == 2
    check(sj.spiral(67, 200), None, 1.0, 200)


def test_comb():
    _, want = check(sj.comb(), None, 1.0, 39)
    assert (want["state"] == 3).sum() == 66 * 39
    check(sj.comb().T.copy(), None, 1.0, 38)
    check(sj.comb()[::-1].copy(), None, 1.0, 39)                          # the spine on the first row


def test_checkerboard_every_pixel_its_own_component():
    _, want = check(sj.checkerboard(), None, 0.0, 1)
    assert (want["size"] == 1).all() and (want["state"] == 3).all()
    check(sj.checkerboard(), None, 0.0, 0)
    check(sj.checkerboard(), None, 1.0, 20)                                # one component at max_diff 1


def test_constant_batch_of_two_one_component_each():
    _, want = check(sj.constant_pair(), None, 1.0, 9099)
    assert (want["labels"] == 0).all() and (want["size"] == 9100).all() and (want["state"] == 0).all()
    check(sj.constant_pair(), None, 0.0, 9100)


# ------------------------------------------------------------------ size boundary
@pytest.mark.parametrize("where", [(16, 64), (32, 128), (0, 0), (47, 139), (0, 139)], **IDS)
@pytest.mark.parametrize("n", [19, 20, 21])
def test_blob_of_exactly_max_size(n, where):
    """A blob of max_size - 1, max_size and max_size + 1 pixels across a tile corner ((16, 64),
    (32, 128)) and in the image's corners."""
    d = sj.blob_image(48, 140, *where, n)
    out, want = check(d, None, 1.0, 20, what=f"blob {n} at {where}")
    blob = d == 50.0
    assert blob.sum() == n and (want["size"][blob] == n).all()
    assert (want["state"][blob] == (3 if n <= 20 else 0)).all()
    rest = ~blob & (want["labels"] == want["labels"][24, 70])  # the background (a blob in an image corner
    assert rest.sum() >= 48 * 140 - 25 and (want["state"][rest] == 0).all()  # may cut a few pixels off it)


def test_max_size_zero_and_whole_image():
    d, e = random_case((2, 67, 131))
    _, want = check(d, e, 1.0, 0, fill=-5.0)
    assert ((want["state"] == 3) == (~np.isfinite(d) & (e == 0))).all()   # nothing but the NaNs
    _, want = check(d, e, 1.0, 67 * 131, fill=-5.0)
    assert (want["state"] != 0).all() and (want["filtered"] == -5.0).all()
    check(d, e, 1.0, 2 ** 31 - 1)


# ------------------------------------------------------------------ values
def test_non_finite_values_and_signed_zero():
    d = np.zeros((40, 90), np.float32)
    d[::2] = -0.0
    d[5, 10:30] = np.inf
    d[17, 60:70] = -np.inf
    d[15:17, 63:65] = np.nan                                              # on a tile corner
    d[30:, 40] = np.nan
    out, want = check(d, None, 0.0, 50, fill=np.nan)
    ok = np.isfinite(d)
    assert (want["size"][ok] == ok.sum()).all() and (want["state"][~ok] == 3).all()
    assert np.array_equal(_bits(out.filtered)[ok], d.view(np.int32)[ok])  # -0.0 stays -0.0
    check(d, None, 0.0, 50, fill=-np.inf)


def test_all_nan_and_all_excluded():
    d = np.full((2, 33, 70), np.nan, np.float32)
    _, want = check(d, None, 1.0, 20, fill=9.0)
    assert (want["labels"] == -1).all() and (want["size"] == 0).all() and (want["state"] == 3).all()
    d = np.ones((2, 33, 70), np.float32)
    e = np.full(d.shape, 2, np.uint8)
    _, want = check(d, e, 1.0, 20, fill=9.0)
    assert (want["labels"] == -1).all() and (want["state"] == 2).all() and (want["filtered"] == 9.0).all()
    check(np.full((1, 1, 1), np.inf, np.float32), None, 0.0, 0)


def test_exclude_as_bool_and_uint8_values_come_back():
    d, e = random_case((1, 130, 70))
    assert set(np.unique(e)) == {0, 1, 2}
    out, want = check(d, e, 1.0, 20)
    st = out.state.cpu().numpy()
    assert (st[e == 1] == 1).all() and (st[e == 2] == 2).all()
    b = kernels.speckle_filter(_dev(d), _dev(e != 0), 20, 1.0, want_labels=True)
    assert_is_judge(b, sj.judge(d, (e != 0).astype(np.uint8), 1.0, 20))


# ------------------------------------------------------------------ plumbing
def test_each_subset_of_outputs():
    d, e = random_case((2, 67, 131))
    want = sj.judge(d, e, 1.0, 20)
    dd, ee = _dev(d), _dev(e)
    for mask in range(8):
        wl, ws, wf = bool(mask & 1), bool(mask & 2), bool(mask & 4)
        out = kernels.speckle_filter(dd, ee, 20, 1.0, want_labels=wl, want_size=ws, want_filtered=wf)
        assert out.disp is dd
        for name, asked in (("labels", wl), ("size", ws), ("state", True), ("filtered", wf)):
            got = getattr(out, name)
            assert (got is not None) == asked, (mask, name)
            if asked:
                assert np.array_equal(_bits(got), _bits(want[name])), (mask, name)
    # state alone NULL through the C entry
    lib = _lib.load()
    n = d.size
    ws_ = torch.empty(2 * n, device=DEV, dtype=torch.int32)
    size = torch.empty(d.shape, device=DEV, dtype=torch.int32)
    kernels.check(lib.lea_disparity_speckle_f32(dd.data_ptr(), ee.data_ptr(), 2, 67, 131, 1.0, 20, 0.0, ws_.data_ptr(),
                                                None, size.data_ptr(), None, None, None), "speckle")
    torch.cuda.synchronize()
    assert np.array_equal(size.cpu().numpy(), want["size"])


def test_non_contiguous_views():
    d, e = random_case((2, 67, 131))
    big = torch.full((2, 134, 133), -3.0, device=DEV)
    big[:, ::2, 1:-1] = _dev(d)
    ebig = torch.full((2, 67, 262), 7, device=DEV, dtype=torch.uint8)
    ebig[:, :, ::2] = _dev(e)
    dv, ev = big[:, ::2, 1:-1], ebig[:, :, ::2]
    assert not dv.is_contiguous() and not ev.is_contiguous()
    out = kernels.speckle_filter(dv, ev, 20, 1.0, want_labels=True)
    assert_is_judge(out, sj.judge(d, e, 1.0, 20))
    t = kernels.speckle_filter(_dev(d[0]).t(), None, 20, 1.0, want_labels=True)
    assert_is_judge(t, sj.judge(d[0].T.copy(), None, 1.0, 20))


def test_guard_bands_stay_untouched():
    d, e = random_case((2, 67, 131))
    B, H, W = d.shape
    n, G = d.size, 1024
    lib = _lib.load()
    dd, ee = _dev(d), _dev(e)
    assert lib.lea_disparity_speckle_workspace_bytes(B, H, W) == 8 * n
    bufs = {"ws": torch.full((2 * n + 2 * G,), -77, device=DEV, dtype=torch.int32),
            "labels": torch.full((n + 2 * G,), -77, device=DEV, dtype=torch.int32),
            "size": torch.full((n + 2 * G,), -77, device=DEV, dtype=torch.int32),
            "state": torch.full((n + 2 * G,), 177, device=DEV, dtype=torch.uint8),
            "filtered": torch.full((n + 2 * G,), -77.0, device=DEV, dtype=torch.float32)}
    p = {k: v.data_ptr() + G * v.element_size() for k, v in bufs.items()}
    kernels.check(lib.lea_disparity_speckle_f32(dd.data_ptr(), ee.data_ptr(), B, H, W, 1.0, 20, 0.0, p["ws"], p["labels"],
                                                p["size"], p["state"], p["filtered"], None), "speckle")
    torch.cuda.synchronize()
    want = sj.judge(d, e, 1.0, 20)
    for k, v in bufs.items():
        a = v.cpu().numpy()
        sentinel = 177 if k == "state" else -77
        assert (a[:G] == sentinel).all() and (a[-G:] == sentinel).all(), k
        if k != "ws":
            assert np.array_equal(_bits(a[G:-G].reshape(d.shape)), _bits(want[k])), k
    assert np.array_equal(_bits(dd), _bits(d)) and np.array_equal(ee.cpu().numpy(), e)   # the inputs too


def test_five_calls_are_bit_identical():
    d, e = random_case((2, 67, 131))
    dd, ee = _dev(d), _dev(e)
    first = kernels.speckle_filter(dd, ee, 20, 1.0, want_labels=True)
    for _ in range(4):
        again = kernels.speckle_filter(dd, ee, 20, 1.0, want_labels=True)
        for name in FIELDS:
            assert torch.equal(getattr(first, name).view(torch.int32) if name == "filtered" else getattr(first, name),
                               getattr(again, name).view(torch.int32) if name == "filtered" else getattr(again, name))
    c = _dev(sj.constant_pair())
    first = kernels.speckle_filter(c, None, 20, 1.0, want_labels=True)
    for _ in range(4):
        again = kernels.speckle_filter(c, None, 20, 1.0, want_labels=True)
        assert torch.equal(first.size, again.size) and torch.equal(first.labels, again.labels)


def test_captured_graph_replays_on_new_data():
    d, e = random_case((2, 67, 131))
    sd, se = _dev(d), _dev(e)
    run = lambda: kernels.speckle_filter(sd, se, 20, 0.5, fill=-1.0, want_labels=True)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    assert_is_judge(out, sj.judge(d, e, 0.5, 20, -1.0), "replay")
    # new data in the same buffers: another field, then a structure that leaves stale labels
    # of the first wrong everywhere
    d2, e2 = sj.random_field((2, 67, 131), seed=99)
    sd.copy_(_dev(d2)), se.copy_(_dev(e2))
    graph.replay()
    assert_is_judge(out, sj.judge(d2, e2, 0.5, 20, -1.0), "replay on new data")
    d3 = np.stack([sj.serpentine(67, 131), sj.comb(67, 131)])
    sd.copy_(_dev(d3)), se.zero_()
    graph.replay()
    assert_is_judge(out, sj.judge(d3, None, 0.5, 20, -1.0), "replay on the structures")


def test_wrapper_refuses_bad_arguments():
    d = torch.zeros(1, 6, 7, device=DEV)
    for kw in (dict(max_diff=-1.0), dict(max_diff=float("nan")), dict(max_diff=float("inf")), dict(max_diff="1"),
               dict(max_size=-1), dict(max_size=2 ** 31), dict(max_size=1.5), dict(max_size=True),
               dict(exclude=torch.zeros(1, 6, 7, device=DEV)), dict(exclude=torch.zeros(1, 6, 6, device=DEV, dtype=torch.uint8)),
               dict(exclude=torch.zeros(1, 6, 7, dtype=torch.uint8)), dict(fill="0")):
        with pytest.raises(ValueError):
            kernels.speckle_filter(d, **kw)
    for bad in (torch.zeros(6, device=DEV), torch.zeros(1, 1, 6, 7, device=DEV), torch.zeros(0, 6, 7, device=DEV)):
        with pytest.raises(ValueError):
            kernels.speckle_filter(bad)
    with pytest.raises(_lib.HipKernelError):
        kernels.speckle_filter(torch.zeros(1, 6, 7, device=DEV, dtype=torch.float64))
    lib = _lib.load()
    rc = lib.lea_disparity_speckle_f32(d.data_ptr(), None, 1, 6, 7, 1.0, 20, 0.0, d.data_ptr(), None, None, None,
                                       d.data_ptr(), None)
    assert rc == _lib.LEA_E_INVALID and b"overlaps" in lib.lea_last_error()


def test_probe_accounts_for_the_call():
    d, _ = random_case((1, 130, 70))
    with kernels.KernelProbe() as probe:
        kernels.speckle_filter(_dev(d))
    s = probe.summary()
    assert s["disparity_speckle"]["launches"] == 1 and s["disparity_speckle"]["bytes"] > 0


# ------------------------------------------------------------------ model level
H, W, MD = 96, 192, 48
REFINE = dict(lam=128.0, sigma=0.1, iterations=2, radius=3, lr_threshold=1.0)
TIGHT = dict(max_size=40, max_diff=0.25)


@functools.lru_cache(maxsize=None)
def _model():
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def _pair(seed):
    return normal(seed, (1, 3, H, W)).to(DEV), normal(seed + 1, (1, 3, H, W)).to(DEV)


def test_forward_refined_without_speckle_is_the_plain_call():
    m = _model()
    left, right = _pair(11)
    with torch.no_grad():
        plain = m.forward_refined(left, right, **REFINE)
        none = m.forward_refined(left, right, speckle=None, **REFINE)
    assert plain._fields == ("disp", "disp_refined", "support", "peak", "disp_right", "state")
    for a, b in zip(plain, none):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("speckle", [{}, TIGHT], ids=["defaults", "tight"])
def test_forward_refined_with_speckle(speckle):
    m = _model()
    left, right = _pair(11)
    with torch.no_grad():
        plain = m(left, right)
        lr = m.forward_lr(left, right, 1.0)
        st = m.forward_with_confidence(left, right, 3)
        out = m.forward_refined(left, right, speckle=speckle, **REFINE)
    assert torch.equal(out.disp, plain) and torch.equal(out.disp_right, lr.disp_right)
    kw = dict(dict(max_size=kernels.SPECKLE_MAX_SIZE, max_diff=kernels.SPECKLE_MAX_DIFF), **speckle)
    want = sj.judge(out.disp.cpu().numpy(), lr.state.cpu().numpy(), kw["max_diff"], kw["max_size"])
    assert np.array_equal(out.state.cpu().numpy(), want["state"])
    print(f"speckle {kw}: {int((want['state'] == 3).sum())} pixels removed, "
          f"{int((lr.state != 0).sum())} flagged by the left-right check")
    by_hand = kernels.fgs_refine(left, plain, st.peak, out.state, 128.0, 0.1, 2, return_support=True)
    assert torch.equal(out.disp_refined.view(torch.int32), by_hand[0].view(torch.int32))
    assert torch.equal(out.support.view(torch.int32), by_hand[1].view(torch.int32))


def test_graphed_refine_with_speckle_replays_the_eager_call():
    m = _model()
    g = m.graphed(1, H, W, refine=dict(REFINE, speckle={}))
    for seed in (21, 31):
        left, right = _pair(seed)
        with torch.no_grad():
            want = m.forward_refined(left, right, speckle={}, **REFINE)
        got = g(left, right)
        assert isinstance(got, kernels.DisparityRefined)
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        lr_state = m.forward_lr(left, right, 1.0).state.cpu().numpy()
        assert np.array_equal(got.state.cpu().numpy(),
                              sj.judge(got.disp.cpu().numpy(), lr_state, 1.0, 200)["state"])


# ------------------------------------------------------------------ scene level
KW = dict(context=8, ramp=8)


def test_speckle_scene_on_a_two_tile_scene():
    m = _model()
    g = golden("c1_sceneflow")
    left = torch.from_numpy(np.ascontiguousarray(g["left_u8"][:H, :300])).to(DEV)
    right = torch.from_numpy(np.ascontiguousarray(g["right_u8"][:H, :300])).to(DEV)
    runner = scene.SceneRunner(m, H, W, tile_batch=2, confidence=True, radius=3, lr_threshold=1.0, **KW)
    assert len(runner.plan(H, 300)) == 2
    res = runner(left, right)
    disp, state = res.disp.cpu().numpy(), res.state.cpu().numpy()
    for kw in ({}, TIGHT):
        full = dict(dict(max_size=200, max_diff=1.0), **kw)
        out = scene.speckle_scene(res, **kw)
        want = sj.judge(disp, state, full["max_diff"], full["max_size"])
        assert out.state.shape == (H, 300) and out.labels is None
        for name in ("size", "state", "filtered"):
            assert np.array_equal(_bits(getattr(out, name)), _bits(want[name])), name
        # refine_scene(speckle=...) refines with that state
        got = scene.refine_scene(res, left, 128.0, 0.1, 2, speckle=kw)
        by_hand = scene.refine_scene(res._replace(state=out.state), left, 128.0, 0.1, 2)
        assert torch.equal(got.view(torch.int32), by_hand.view(torch.int32))
    assert torch.equal(scene.refine_scene(res, left, 128.0, 0.1, 2, speckle=None).view(torch.int32),
                       scene.refine_scene(res, left, 128.0, 0.1, 2).view(torch.int32))


def test_predict_cli_speckle(tmp_path):
    """A 96 x 300 sceneflow-layout pair (two tiles): --speckle adds its two files, at the image's
    size under --scene 1, with the flags of --lr_check as walls, and moves nothing else; with
    --refine 1 the refinement is the one that excludes the removed pixels."""
    from PIL import Image
    from leastereo_amd import predict as P
    g = golden("c1_sceneflow")
    for side in ("left", "right"):
        d = tmp_path / "frames_finalpass" / "S" / side
        d.mkdir(parents=True)
        Image.fromarray(g[side + "_u8"][:H, :300]).save(d / "0001.png")
    (tmp_path / "list.txt").write_text("S/left/0001.png\n")
    torch.save({"state_dict": {"module." + k: v for k, v in state_dict().items()}}, tmp_path / "ckpt.pth")
    base = ["--sceneflow=1", f"--maxdisp={MD}", "--crop_height=96", "--crop_width=192",
            f"--data_path={tmp_path}/", f"--test_list={tmp_path}/list.txt", f"--resume={tmp_path}/ckpt.pth",
            "--scene", "1", "--scene_context=8", "--scene_ramp=8", "--scene_batch=2", "--lr_check=1", "--refine=1",
            "--refine_lambda=128", "--refine_sigma=0.1", "--refine_iters=2", "--conf_radius=3"]
    assert P.main(base + [f"--save_path={tmp_path}/plain/"]) == 0
    assert P.main(base + [f"--save_path={tmp_path}/speckle/", "--speckle", "60", "--speckle_diff=0.5"]) == 0
    new = ("0_speckle.png", "0_despeckled.npy")
    assert sorted(p.name for p in (tmp_path / "speckle").iterdir()) == sorted(
        [p.name for p in (tmp_path / "plain").iterdir()] + list(new))
    for same in ("0.npy", "0_right.npy", "0_filled.npy"):
        assert np.array_equal(np.load(tmp_path / "plain" / same), np.load(tmp_path / "speckle" / same)), same
    disp = np.load(tmp_path / "speckle" / "0.npy")
    left, right = P.load_images(*P.sceneflow_names(f"{tmp_path}/", "S/left/0001.png\n")[:2])
    runner = scene.SceneRunner(_model(), H, W, tile_batch=2, confidence=True, radius=3, lr_threshold=1.0, **KW)
    res = runner(left, right)
    assert np.array_equal(disp, res.disp.cpu().numpy())
    want = sj.judge(disp, res.state.cpu().numpy(), 0.5, 60)
    got = np.load(tmp_path / "speckle" / "0_despeckled.npy")
    assert got.shape == (H, 300) and got.dtype == np.float32
    assert np.array_equal(got.view(np.int32), want["filtered"].view(np.int32))
    png = np.asarray(Image.open(tmp_path / "speckle" / "0_speckle.png"))
    assert png.shape == (H, 300) and np.array_equal(png == 255, want["state"] == 3) and (want["state"] == 3).any()
    refined = scene.refine_scene(res, left, 128.0, 0.1, 2, speckle=dict(max_size=60, max_diff=0.5))
    assert np.array_equal(np.load(tmp_path / "speckle" / "0_refined.npy"), refined.cpu().numpy())
    assert not np.array_equal(np.load(tmp_path / "plain" / "0_refined.npy"), refined.cpu().numpy())
    # without --scene and the other flags: on the crop, no walls
    pair = base[:7] + [f"--save_path={tmp_path}/pair/", "--speckle=60"]
    assert P.main(pair) == 0
    crop = np.load(tmp_path / "pair" / "0.npy")
    want = sj.judge(crop, None, 1.0, 60)
    assert np.array_equal(np.load(tmp_path / "pair" / "0_despeckled.npy").view(np.int32), want["filtered"].view(np.int32))
    assert np.asarray(Image.open(tmp_path / "pair" / "0_speckle.png")).shape == crop.shape


def test_blob_across_the_tile_cut_is_judged_at_its_whole_size():
    """Two rows of a blob that overhangs the overlap of the two tiles of a 96 x 300 scene by 12
    columns on either side: at scene size it is above max_size = 200 and stays; either tile
    alone sees 24 pixels fewer, at most 200, and would remove it."""
    m = _model()
    runner = scene.SceneRunner(m, H, W, tile_batch=2, **KW)
    plan = runner.plan(H, 300)
    assert len(plan) == 2 and plan.xs[0] == 0 and 0 < plan.xs[1] < W
    a, b = plan.xs[1] - 12, W + 12                             # the overlap is plan.xs[1] .. W
    d = np.full((H, 300), 10.0, np.float32)
    d[40:42, a:b] = 30.0
    res = scene.SceneResult(disp=_dev(d))
    out = scene.speckle_scene(res)
    want = sj.judge(d, None, 1.0, 200)
    for name in ("size", "state", "filtered"):
        assert np.array_equal(_bits(getattr(out, name)), _bits(want[name])), name
    assert 2 * (b - a) > 200 and (want["size"][40:42, a:b] == 2 * (b - a)).all() and (want["state"] == 0).all()
    for x0, x1 in ((0, W), (plan.xs[1], plan.xs[1] + W)):      # what either tile alone would do
        part = kernels.speckle_filter(_dev(d[:, x0:x1].copy()))
        blob = d[:, x0:x1] == 30.0
        assert 0 < blob.sum() <= 200 and (part.state.cpu().numpy()[blob] == 3).all()
