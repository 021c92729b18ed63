"""The disparity refinement on the GPU (lea_disparity_refine_f32, kernels.fgs_refine,
LEAStereo.forward_refined / graphed(refine=...), scene.refine_scene, predict --refine).

Accuracy is judged against tests/refine_judge.py's float64 restatement of the header's
definition.  The bar, none of it taken from what the kernel gives, is the photometric
section's: max(4 x E32, 8 ulp(max |disp|)), E32 being the same judge run in float32 on that very
case; ``support`` gets the same bar at its own magnitude.  No pixel is left out, except in the
threshold test the pixels whose float64 support lies within a factor of 10 of the 1e-30
threshold, where either branch is right.  Each case prints its figures before it asserts
(pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels, scene
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from tests import refine_judge as rj
from tests.golden_util import golden, normal, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, C, H, W): lines of length 1 and 2, both sides of a wave (64 lines), of a 32-column chunk
# and of a 16-row batch, a partial wave of lines, and a carry across 48 chunks
SHAPES = [(2, 3, 5, 7), (1, 1, 1, 64), (1, 3, 2, 1), (1, 3, 65, 2), (1, 3, 37, 131), (2, 1, 5, 257),
          (1, 4, 64, 65), (1, 3, 3, 1513)]
PARAMS = [(lam, sigma, T) for lam in (4.0, 128.0, 8000.0) for sigma in (0.1, 0.5) for T in (1, 3)]
IDS = dict(ids=lambda s: "x".join(map(str, s)))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)  # a copy: the references are read-only


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def reference(shape, lam, sigma, T):
    """The inputs of a case and both judges' results, made once."""
    guide, disp, conf = rj.make_case(shape, seed=sum(shape))
    want = rj.refine64(guide, disp, conf, None, lam, sigma, T)
    w32 = rj.refine32(guide, disp, conf, None, lam, sigma, T)
    for v in (guide, disp, conf, *want.values(), *w32.values()):
        v.setflags(write=False)
    return guide, disp, conf, want, w32


@pytest.mark.parametrize("lam,sigma,T", PARAMS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_refined_and_support_against_fp64(shape, lam, sigma, T):
    guide, disp, conf, want, w32 = reference(shape, lam, sigma, T)
    assert want["solved"].all() and w32["solved"].all()
    refined, support = kernels.fgs_refine(_dev(guide), _dev(disp), _dev(conf), None, lam, sigma, T,
                                          return_support=True)
    bar, e32 = rj.bar(want["refined"], w32["refined"], np.abs(disp).max())
    bar_s, e32_s = rj.bar(want["den"], w32["den"], want["den"].max())
    err = float(np.abs(refined.cpu().numpy().astype(np.float64) - want["refined"]).max())
    err_s = float(np.abs(support.cpu().numpy().astype(np.float64) - want["den"]).max())
    print(f"{shape} lambda {lam} sigma {sigma} T {T}: refined err {err:.3e} E32 {e32:.3e} ratio "
          f"{err / e32 if e32 else float('nan'):.2f} bar {bar:.3e}; support err {err_s:.3e} E32 {e32_s:.3e} "
          f"bar {bar_s:.3e}")
    assert refined.shape == support.shape == shape[:1] + shape[2:]
    assert err <= bar
    assert err_s <= bar_s


@pytest.mark.parametrize("lam,T", [(0.05, 1), (0.02, 2)])
def test_threshold_branch(lam, T):
    """Evidence on a 6-pixel frame only, a small lambda: the support underflows inside, and
    those pixels keep their disparity bit for bit (0 for a NaN)."""
    B, C, H, W = shape = (1, 1, 72, 130)
    rng = np.random.default_rng(7)
    guide, _ = rj.piecewise_guide(rng, B, C, H, W)
    disp = rng.uniform(0, 90, size=(B, H, W)).astype(np.float32)
    disp[0, 30:40, 50:60] = np.nan
    disp[0, 36, 64] = -np.inf
    conf = np.ones((B, H, W), dtype=np.float32)
    conf[:, 6:-6, 6:-6] = 0
    sigma = 0.5
    want = rj.refine64(guide, disp, conf, None, lam, sigma, T)
    w32 = rj.refine32(guide, disp, conf, None, lam, sigma, T)
    refined, support = kernels.fgs_refine(_dev(guide), _dev(disp), _dev(conf), None, lam, sigma, T,
                                          return_support=True)
    refined, support = refined.cpu().numpy(), support.cpu().numpy()
    near = (want["den"] > 1e-31) & (want["den"] < 1e-29)
    keep = ~near
    solved = want["solved"]
    print(f"lambda {lam} T {T}: judge puts {100 * (~solved).mean():.1f} % on the fallback, "
          f"{100 * near.mean():.1f} % within a factor 10 of the threshold")
    assert solved.any() and (~solved).mean() > 0.1 and near.mean() <= 0.05
    assert np.array_equal((support > rj.DEN_MIN)[keep], solved[keep])
    assert np.array_equal(w32["solved"][keep], solved[keep])
    fb = keep & ~solved
    assert np.isnan(disp[fb]).any() and np.isinf(disp[fb]).any()
    assert np.array_equal(refined[fb].view(np.int32), want["fallback"][fb].view(np.int32))
    assert np.isfinite(refined).all() and np.isfinite(support).all()
    ok = keep & solved
    bar, e32 = rj.bar(want["refined"][ok], w32["refined"][ok], np.nanmax(np.abs(disp[np.isfinite(disp)])))
    err = float(np.abs(refined[ok].astype(np.float64) - want["refined"][ok]).max())
    bar_s, e32_s = rj.bar(want["den"][keep], w32["den"][keep], want["den"].max())
    err_s = float(np.abs(support[keep].astype(np.float64) - want["den"][keep]).max())
    print(f"  refined err {err:.3e} E32 {e32:.3e} bar {bar:.3e}; support err {err_s:.3e} bar {bar_s:.3e}")
    assert err <= bar and err_s <= bar_s


def test_a_batch_item_without_evidence_keeps_its_disparity():
    guide, disp, conf = rj.make_case((2, 3, 37, 131), seed=9)
    disp, conf = disp.copy(), conf.copy()
    conf[1] = 0
    disp[1, 3, 5], disp[1, 20, 100], disp[1, 36, 130] = np.nan, np.inf, -np.inf
    refined, support = kernels.fgs_refine(_dev(guide), _dev(disp), _dev(conf), None, 128.0, 0.1, 3,
                                          return_support=True)
    want1 = np.where(np.isfinite(disp[1]), disp[1], np.float32(0))
    assert np.array_equal(_bits(refined[1]), want1.view(np.int32))
    assert np.array_equal(_bits(support[1]), np.zeros((37, 131), dtype=np.int32))
    alone = kernels.fgs_refine(_dev(guide[:1]), _dev(disp[:1]), _dev(conf[:1]), None, 128.0, 0.1, 3,
                               return_support=True)
    assert same_bits(refined[0], alone[0][0]) and same_bits(support[0], alone[1][0])
    assert float(support[0].min()) > 0


def test_poison_under_zero_weight_never_enters_the_arithmetic():
    guide, disp, conf = rj.make_case((2, 3, 37, 131), seed=10)
    rng = np.random.default_rng(10)
    disp, conf = disp.copy(), conf.copy()
    exclude = (rng.uniform(size=disp.shape) < 0.2).astype(np.uint8)
    poison = np.array([np.nan, np.inf, -np.inf, -5.0, -1e30], dtype=np.float32)
    ex = exclude != 0
    disp[ex] = poison[rng.integers(0, 5, size=int(ex.sum()))]
    bad_conf = (rng.uniform(size=disp.shape) < 0.1) & ~ex
    conf[bad_conf] = np.array([np.nan, -1.0, -np.inf, np.inf], dtype=np.float32)[rng.integers(0, 4, size=int(bad_conf.sum()))]
    nan_disp = (rng.uniform(size=disp.shape) < 0.05) & ~ex & ~bad_conf  # not finite, not excluded
    disp[nan_disp] = np.nan
    got = kernels.fgs_refine(_dev(guide), _dev(disp), _dev(conf), _dev(exclude), 128.0, 0.1, 3, return_support=True)
    dead = ex | bad_conf | nan_disp
    clean_d, clean_c = np.where(dead, np.float32(0), disp), np.where(dead, np.float32(0), conf)
    want = kernels.fgs_refine(_dev(guide), _dev(clean_d), _dev(clean_c), None, 128.0, 0.1, 3, return_support=True)
    for g, w in zip(got, want):
        assert torch.isfinite(g).all()
        assert same_bits(g, w)
    assert float(got[1].min()) > 1e-30  # every pixel was solved: none of them is the fallback


def test_views_and_the_state_of_lr_check_go_as_they_are():
    B, C, H, W = 2, 3, 37, 131
    guide, disp, conf = rj.make_case((B, 6, H, W), seed=11)
    big = _dev(guide)
    view = big[:, 1:4]
    assert view.stride(0) == 6 * H * W and not view.is_contiguous()
    dl = _dev(disp)
    rng = np.random.default_rng(11)
    dr = _dev((disp + rng.normal(0, 1.0, size=disp.shape)).astype(np.float32))
    state = kernels.lr_check(dl, dr, 1.0, want_filled=False).state
    assert 0 < int((state != 0).sum()) < state.numel()
    got = kernels.fgs_refine(view, dl, _dev(conf), state, 128.0, 0.1, 2, return_support=True)
    want = kernels.fgs_refine(view.contiguous(), dl, _dev(conf), state.clone(), 128.0, 0.1, 2, return_support=True)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    # a bool mask is the same mask
    again = kernels.fgs_refine(view, dl, _dev(conf), state != 0, 128.0, 0.1, 2)
    assert same_bits(again, want[0])
    ref = rj.refine64(guide[:, 1:4], disp, conf, state.cpu().numpy(), 128.0, 0.1, 2)
    r32 = rj.refine32(guide[:, 1:4], disp, conf, state.cpu().numpy(), 128.0, 0.1, 2)
    bar, e32 = rj.bar(ref["refined"], r32["refined"], np.abs(disp).max())
    err = float(np.abs(got[0].cpu().numpy().astype(np.float64) - ref["refined"]).max())
    print(f"views: err {err:.3e} E32 {e32:.3e} bar {bar:.3e}")
    assert ref["solved"].all() and err <= bar


@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_nothing_is_written_outside_the_outputs_and_the_workspace(shape):
    """refined, support and the workspace inside larger sentinel-filled buffers."""
    lam, sigma, T = 128.0, 0.1, 3
    guide, disp, conf, want, w32 = reference(shape, lam, sigma, T)
    B, C, H, W = shape
    n, pad, sent = B * H * W, 1024, -12345.0
    lib = _lib.load()
    assert lib.lea_disparity_refine_workspace_bytes(B, H, W) == 28 * n
    outs = torch.full((2 * n + 3 * pad,), sent, device=DEV)
    ws = torch.full((7 * n + 2 * pad,), sent, device=DEV)
    g, d, c = _dev(guide), _dev(disp), _dev(conf)
    refined, support = outs[pad:pad + n], outs[2 * pad + n:2 * pad + 2 * n]
    _lib.check(lib.lea_disparity_refine_f32(g.data_ptr(), C * H * W, d.data_ptr(), c.data_ptr(), None, B, C, H, W, lam,
                                            sigma, T, ws[pad:].data_ptr(), refined.data_ptr(), support.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "lea_disparity_refine_f32")
    for t in (outs[:pad], outs[pad + n:2 * pad + n], outs[2 * pad + 2 * n:], ws[:pad], ws[pad + 7 * n:]):
        assert bool((t == sent).all())
    direct = kernels.fgs_refine(g, d, c, None, lam, sigma, T, return_support=True)
    assert same_bits(refined.view(B, H, W), direct[0]) and same_bits(support.view(B, H, W), direct[1])
    # support = NULL: the same refined, the second buffer untouched
    outs.fill_(sent)
    _lib.check(lib.lea_disparity_refine_f32(g.data_ptr(), C * H * W, d.data_ptr(), c.data_ptr(), None, B, C, H, W, lam,
                                            sigma, T, ws[pad:].data_ptr(), refined.data_ptr(), None,
                                            torch.cuda.current_stream().cuda_stream), "lea_disparity_refine_f32")
    assert same_bits(refined.view(B, H, W), direct[0]) and bool((outs[pad + n:] == sent).all())


def test_two_calls_and_a_graph_replay_give_the_same_bits():
    guide, disp, conf = rj.make_case((2, 3, 37, 131), seed=12)
    g, d, c = _dev(guide), _dev(disp), _dev(conf)
    a = kernels.fgs_refine(g, d, c, None, 8000.0, 0.1, 3, return_support=True)
    b = kernels.fgs_refine(g, d, c, None, 8000.0, 0.1, 3, return_support=True)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kernels.fgs_refine(g, d, c, None, 8000.0, 0.1, 3, return_support=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = kernels.fgs_refine(g, d, c, None, 8000.0, 0.1, 3, return_support=True)
    for _ in range(2):
        out[0].zero_(), out[1].zero_()
        graph.replay()
        assert same_bits(out[0], a[0]) and same_bits(out[1], a[1])


def test_wrapper_refusals_reach_python():
    g, d = torch.zeros(1, 3, 6, 7, device=DEV), torch.zeros(1, 6, 7, device=DEV)
    for kw in (dict(lam=0.0), dict(sigma=-1.0), dict(iterations=9), dict(iterations=0), dict(lam=float("nan"))):
        with pytest.raises(ValueError):
            kernels.fgs_refine(g, d, **kw)
    with pytest.raises(ValueError):
        kernels.fgs_refine(torch.zeros(1, 5, 6, 7, device=DEV), d)
    with pytest.raises(ValueError):
        kernels.fgs_refine(g, d[:, :5])
    with pytest.raises(ValueError):
        kernels.fgs_refine(g, d, exclude=torch.zeros(1, 6, 7, device=DEV))
    lib = _lib.load()
    rc = lib.lea_disparity_refine_f32(g.data_ptr(), 126, d.data_ptr(), None, None, 1, 3, 6, 7, 1.0, 1.0, 1,
                                      d.data_ptr(), d.data_ptr(), None, None)
    assert rc == _lib.LEA_E_INVALID and b"overlaps" in lib.lea_last_error()


# ------------------------------------------------------------------ model level
H, W, MD = 96, 192, 48
REFINE = dict(lam=128.0, sigma=0.1, iterations=2, radius=3, lr_threshold=1.0)


@functools.lru_cache(maxsize=None)
def _model():
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def _pair(seed):
    return normal(seed, (1, 3, H, W)).to(DEV), normal(seed + 1, (1, 3, H, W)).to(DEV)


def test_forward_refined():
    m = _model()
    left, right = _pair(11)
    with torch.no_grad():
        plain = m(left, right)
        st = m.forward_with_confidence(left, right, 3)
        lr = m.forward_lr(left, right, 1.0)
        out = m.forward_refined(left, right, **REFINE)
    assert isinstance(out, kernels.DisparityRefined)
    assert torch.equal(out.disp, plain)
    assert torch.equal(out.peak, st.peak)
    assert torch.equal(out.disp_right, lr.disp_right) and torch.equal(out.state, lr.state)
    want = kernels.fgs_refine(left, plain, st.peak, lr.state, 128.0, 0.1, 2, return_support=True)
    assert same_bits(out.disp_refined, want[0]) and same_bits(out.support, want[1])
    assert torch.isfinite(out.disp_refined).all() and out.disp_refined.shape == plain.shape
    assert not torch.equal(out.disp_refined, plain)
    m.train()
    try:
        with pytest.raises(RuntimeError, match="inference only"):
            m.forward_refined(left, right)
    finally:
        m.eval()
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_refined(left.clone().requires_grad_(), right)


def test_graphed_refine_replays_the_eager_call():
    m = _model()
    with pytest.raises(ValueError):
        m.graphed(1, H, W, confidence=True, refine={})
    with pytest.raises(ValueError):
        m.graphed(1, H, W, lr_threshold=1.0, refine={})
    g = m.graphed(1, H, W, refine=REFINE)
    for seed in (21, 31):
        left, right = _pair(seed)
        with torch.no_grad():
            want = m.forward_refined(left, right, **REFINE)
        got = g(left, right)
        assert isinstance(got, kernels.DisparityRefined)
        for a, b in zip(got, want):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ scene level
KW = dict(context=8, ramp=8)


def _golden_pair(h, w):
    g = golden("c1_sceneflow")
    return (torch.from_numpy(np.ascontiguousarray(g["left_u8"][:h, :w])).to(DEV),
            torch.from_numpy(np.ascontiguousarray(g["right_u8"][:h, :w])).to(DEV))


def test_refine_scene_runs_once_on_the_blended_maps():
    m = _model()
    left, right = _golden_pair(H, 300)
    runner = scene.SceneRunner(m, H, W, tile_batch=2, confidence=True, radius=3, lr_threshold=1.0, **KW)
    assert len(runner.plan(H, 300)) == 2
    res = runner(left, right)
    guide = kernels.standardize_crop_u8(left, right, H, 300)[0]  # the scene, its own statistics
    want = kernels.fgs_refine(guide, res.disp[None], res.peak[None], res.state[None], 128.0, 0.1, 2,
                              return_support=True)
    got = scene.refine_scene(res, left, 128.0, 0.1, 2, return_support=True)
    assert got[0].shape == got[1].shape == (H, 300)
    assert same_bits(got[0], want[0][0]) and same_bits(got[1], want[1][0])
    assert same_bits(scene.refine_scene(res, left.cpu().numpy(), 128.0, 0.1, 2), want[0][0])
    # the defaults are fgs_refine's; a result without peak or state refines with neither
    bare = scene.SceneResult(disp=res.disp)
    assert same_bits(scene.refine_scene(bare, left), kernels.fgs_refine(guide, res.disp[None])[0])
    with pytest.raises(ValueError):
        scene.refine_scene(res, left[:, :200])


def test_predict_cli_scene_refine(tmp_path):
    """A 96 x 300 sceneflow-layout pair (two tiles): --scene 1 --refine 1 adds the three files, at
    the image's size, and moves nothing else."""
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
            "--scene", "1", "--scene_context=8", "--scene_ramp=8", "--scene_batch=2"]
    assert P.main(base + [f"--save_path={tmp_path}/plain/"]) == 0
    assert P.main(base + [f"--save_path={tmp_path}/refine/", "--refine", "1", "--refine_lambda=128",
                          "--refine_sigma=0.1", "--refine_iters=2", "--conf_radius=3"]) == 0
    new = ("0_refined.npy", "0_refined.png", "0_support.png")
    assert sorted(p.name for p in (tmp_path / "refine").iterdir()) == sorted(
        [p.name for p in (tmp_path / "plain").iterdir()] + list(new))
    assert np.array_equal(np.load(tmp_path / "plain" / "0.npy"), np.load(tmp_path / "refine" / "0.npy"))
    refined = np.load(tmp_path / "refine" / "0_refined.npy")
    assert refined.shape == (H, 300) and refined.dtype == np.float32 and np.isfinite(refined).all()
    assert np.asarray(Image.open(tmp_path / "refine" / "0_refined.png")).shape[:2] == (H, 300)
    assert np.asarray(Image.open(tmp_path / "refine" / "0_support.png")).shape == (H, 300)
    left, right = P.load_images(*P.sceneflow_names(f"{tmp_path}/", "S/left/0001.png\n")[:2])
    runner = scene.SceneRunner(_model(), H, W, tile_batch=2, confidence=True, radius=3, lr_threshold=1.0, **KW)
    want = scene.refine_scene(runner(left, right), left, 128.0, 0.1, 2)
    assert np.array_equal(refined, want.cpu().numpy())
    # without --scene: one forward_refined on the crop, its maps cropped like the disparity
    assert P.main(base[:7] + [f"--save_path={tmp_path}/pair/", "--refine=1"]) == 0
    crop = np.load(tmp_path / "pair" / "0.npy").shape
    assert crop != (H, 300) and np.load(tmp_path / "pair" / "0_refined.npy").shape == crop
    assert np.asarray(Image.open(tmp_path / "pair" / "0_support.png")).shape == crop
