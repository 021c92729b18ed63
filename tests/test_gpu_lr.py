"""The left-right check on the GPU: the right head (lea_disparity_regression_right) against an
fp64 judge, the check and fill (lea_disparity_lr_check) bit for bit against a numpy judge,
the three launches on an occlusion scene, LEAStereo.forward_lr / graphed(lr_threshold=...)
and predict --lr_check.

The right head's judge is written here: F.interpolate (trilinear, align_corners=False) to
the full U [MD, 3H3, 3W3], a gather along xr + od with the out-of-view candidates at -inf,
softmax, expectation.  Bars (none taken from what the kernel gives), the sibling head's own
(test_gpu_disp_stats.py): the max abs error against fp64 is at most
max(4 x E_cpu32, 32 ulp(MD)), E_cpu32 being the same judge run in float32 on the CPU for
that very case; the hardware-exp dtype gets the same bar times R = max(1, err(plain fast
disp) / err(plain f32 disp)), both of the existing left entry against fp64 on that case.
No pixel is left out.  Each case prints its figures before it asserts (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from leastereo_amd import _lib, kernels
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from tests.golden_util import golden, normal, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, D3, H3, W3): the smallest shapes at which each code path can go wrong
SHAPES = [(2, 4, 5, 7),      # odd sizes, batch stride, most pixels truncated
          (1, 8, 3, 90),     # Wo = 270 > 256: the diagonal crosses a W tile boundary
          (1, 64, 4, 90),    # the product depth
          (1, 88, 3, 90),    # MD = 264 ~ Wo: nearly every pixel truncated; C5's depth
          (2, 5, 4, 6),      # unconfigured depth: the generic form
          (1, 8, 2, 7)]      # MD = 24 > Wo = 21
SCALES = (1, 3, 20)          # flat to sharp
IDS = dict(ids=lambda s: "x".join(map(str, s)))


def make_cost(shape, scale):
    b, d3, h3, w3 = shape
    g = torch.Generator().manual_seed(0)
    return torch.randn(b, 1, d3, h3, w3, generator=g) * scale


def judge_right(cost, dtype):
    """disp_right [B, 3H3, 3W3] of the header's definition (torch CPU, ``dtype``)."""
    x = cost.to(dtype)
    b, _, d3, h3, w3 = x.shape
    md, ho, wo = 3 * d3, 3 * h3, 3 * w3
    u = F.interpolate(x, size=(md, ho, wo), mode="trilinear", align_corners=False)[:, 0]
    src = torch.arange(wo).view(1, wo) + torch.arange(md).view(md, 1)          # xr + od
    diag = u.gather(3, src.clamp(max=wo - 1).view(1, md, 1, wo).expand(b, md, ho, wo))
    diag = torch.where((src <= wo - 1).view(1, md, 1, wo), -diag, torch.full_like(diag, -float("inf")))
    return (F.softmax(diag, dim=1) * torch.arange(md, dtype=dtype).view(1, md, 1, 1)).sum(1)


def judge_plain(cost):
    x = cost.double()
    md = 3 * x.shape[2]
    u = F.interpolate(x, size=(md, 3 * x.shape[3], 3 * x.shape[4]), mode="trilinear", align_corners=False)[:, 0]
    return (F.softmax(-u, dim=1) * torch.arange(md, dtype=torch.float64).view(1, md, 1, 1)).sum(1)


@functools.lru_cache(None)
def reference(shape, scale):
    """Per (shape, scale), computed once and left unchanged: the cost, the fp64 judge, its
    float32 restatement's error and the plain entry's two errors against fp64."""
    cost = make_cost(shape, scale)
    j64 = judge_right(cost, torch.float64)
    e_cpu = float((judge_right(cost, torch.float32).double() - j64).abs().max())
    dev = cost.to(DEV)
    md = 3 * shape[1]
    p64 = judge_plain(cost)
    err = {fast: float((kernels.disparity_regression(dev, md, fast).cpu().double() - p64).abs().max())
           for fast in (False, True)}
    return dict(cost=dev, j64=j64, e_cpu=e_cpu, R=max(1.0, err[True] / err[False]))


def ulp_of(x):
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("fast", [False, True], ids=["f32", "hwexp"])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_right_against_fp64(shape, scale, fast):
    ref = reference(shape, scale)
    md = 3 * shape[1]
    got = kernels.disparity_regression_right(ref["cost"], md, fast).cpu()
    assert got.shape == ref["j64"].shape and got.dtype == torch.float32
    R = ref["R"] if fast else 1.0
    e_gpu = float((got.double() - ref["j64"]).abs().max())
    bar = max(4 * ref["e_cpu"], 32 * ulp_of(md)) * R
    print(f"{shape} x{scale} fast={int(fast)} disp_right gpu {e_gpu:.3e} cpu32 {ref['e_cpu']:.3e} bar {bar:.3e} "
          f"R {R:.2f} gpu/cpu32 {e_gpu / max(ref['e_cpu'], 1e-30):.2f}")
    assert torch.isfinite(got).all()
    assert e_gpu <= bar, (e_gpu, bar)
    assert bool((got[..., -1] == 0).all()), "the last column has one candidate: exactly 0"


# ------------------------------------------------------------------ analytic cases
@pytest.mark.parametrize("fast", [False, True], ids=["f32", "hwexp"])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_right_constant_cost(shape, fast):
    """Every exponential is 1: the mean of 0 .. n - 1, n = min(MD, Wo - xr)."""
    b, d3, h3, w3 = shape
    md, wo = 3 * d3, 3 * w3
    got = kernels.disparity_regression_right(torch.full((b, 1, d3, h3, w3), 0.7, device=DEV), md, fast).cpu()
    n = torch.clamp(wo - torch.arange(wo), max=md).double()
    want = ((n - 1) / 2).view(1, 1, wo).expand_as(got)
    assert float((got.double() - want).abs().max()) <= 4 * ulp_of(md)
    assert bool((got[..., -1] == 0).all())


@pytest.mark.parametrize("fast", [False, True], ids=["f32", "hwexp"])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_right_minimum_is_over_the_candidates_in_view(shape, fast):
    """Plane D3 - 1 at -300, the rest 0.  Where the last plane is out of view every in-view
    U is 0 and the answer is (n - 1) / 2; a shift taken over all planes (-300) makes every
    exponential there underflow (s = 0: NaN)."""
    b, d3, h3, w3 = shape
    md, wo = 3 * d3, 3 * w3
    cost = torch.zeros(b, 1, d3, h3, w3)
    cost[:, :, d3 - 1] = -300.0
    got = kernels.disparity_regression_right(cost.to(DEV), md, fast).cpu()
    assert torch.isfinite(got).all()
    want = judge_right(cost, torch.float64)
    xr = torch.arange(wo)
    out = xr > wo - 1 - 3 * (d3 - 1) + 1  # no candidate there touches plane D3 - 1
    assert bool(out.any())
    n = torch.clamp(wo - xr, max=md).double()
    assert float((want[..., out] - ((n - 1) / 2)[out]).abs().max()) <= 1e-12  # the judge agrees it is flat there
    assert float((got.double() - want)[..., out].abs().max()) <= 4 * ulp_of(md)


def test_right_refusals_reach_python():
    cost = torch.zeros(1, 1, 4, 2, 2, device=DEV)
    with pytest.raises(_lib.HipKernelError, match="maxdisp"):
        kernels.disparity_regression_right(cost, 13)
    with pytest.raises(_lib.HipKernelError, match="threshold"):
        kernels.lr_check(torch.zeros(1, 2, 2, device=DEV), torch.zeros(1, 2, 2, device=DEV), 0.0)


# ------------------------------------------------------------------ check and fill
def judge_check(dl, dr, thr):
    """state (uint8) and disp_filled of the header's definition, numpy float32."""
    f = np.float32
    b, h, w = dl.shape
    with np.errstate(invalid="ignore"):
        xi = np.floor(((np.arange(w, dtype=f) - dl).astype(f) + f(0.5)).astype(f))
        oov = (xi < 0) | (xi > w - 1)
        at = np.take_along_axis(dr, np.clip(np.nan_to_num(xi, nan=0.0, posinf=0.0, neginf=0.0), 0, w - 1).astype(np.int64), 2)
        bad = ~np.isfinite(dl) | ~(np.abs((dl - at).astype(f)) <= f(thr))
    state = np.where(oov, 2, np.where(bad, 1, 0)).astype(np.uint8)
    # the nearest state-0 pixel at or before / at or after each pixel, as indices (-1 / w: none)
    x = np.arange(w)
    good = state == 0
    li = np.maximum.accumulate(np.where(good, x, -1), axis=2)
    ri = np.minimum.accumulate(np.where(good, x, w)[..., ::-1], axis=2)[..., ::-1]
    lv = np.take_along_axis(dl, np.clip(li, 0, w - 1), 2)
    rv = np.take_along_axis(dl, np.clip(ri, 0, w - 1), 2)
    both = np.where(rv < lv, rv, lv)
    fill = np.where(li < 0, np.where(ri >= w, dl, rv), np.where(ri >= w, lv, both))
    filled = np.where(good, dl, fill).astype(f)
    return state, filled


WIDTHS = (1, 2, 63, 64, 65, 257, 1513)
PATTERNS = ("all", "none", "first", "last", "alternating", "runs", "nan_negative")
LB, LH = 2, 3


def make_pair(w, pattern):
    """disp_left / disp_right [2, 3, W] in multiples of 1/8 (x - dL + 0.5 and dL - dR exact in
    f32) whose consistent pixels follow ``pattern``.  dL in [0, 0.5] maps pixel x onto xi = x,
    so disp_right[x] alone decides pixel x: dL + 0.5 (consistent) or dL + 3 (not)."""
    rng = np.random.RandomState(w * 31 + PATTERNS.index(pattern))
    x = np.arange(w)
    rows = np.arange(LB * LH).reshape(LB, LH, 1)
    dl = (((x * 7 + rows * 3) % 5) / 8).astype(np.float32)
    ok = np.zeros((LB, LH, w), bool)
    if pattern == "all":
        ok[:] = True
    elif pattern == "first":
        ok[..., 0] = True
    elif pattern == "last":
        ok[..., -1] = True
    elif pattern == "alternating":
        ok = ((x + rows) % 2 == 0)
    elif pattern in ("runs", "nan_negative"):
        # runs of flagged pixels longer than a lane's segment, a wave's 64 and a chunk's 256
        ok = rng.rand(LB, LH, w) < 0.5
        for lo, n in ((3, 70), (100, 300), (700, 530), (1300, 213)):
            ok[rng.randint(LB), rng.randint(LH), lo:lo + n] = False
        ok[0, 0, : w // 2] = False
        ok[1, 2, w // 3:] = False
    dr = np.where(ok, dl + np.float32(0.5), dl + np.float32(3.0)).astype(np.float32)
    if pattern == "nan_negative":
        hit = rng.rand(LB, LH, w)
        dl = dl.copy()
        dl[hit < 0.05] = np.nan
        dl[(hit >= 0.05) & (hit < 0.10)] = -5.25          # xi = x + 5 (+ a tie-free .75): beyond W - 1 at the right edge
        dl[(hit >= 0.10) & (hit < 0.15)] = 7.5            # xi < 0 at the left edge, another pixel's target inside
        dl[(hit >= 0.15) & (hit < 0.17)] = np.inf
        dl[(hit >= 0.17) & (hit < 0.19)] = -np.inf
    return np.ascontiguousarray(dl), dr, ok


@functools.lru_cache(None)
def check_reference(w, pattern):
    dl, dr, ok = make_pair(w, pattern)
    state, filled = judge_check(dl, dr, 1.0)
    return dl, dr, ok, state, filled


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("w", WIDTHS)
def test_check_and_fill_bit_exact(w, pattern):
    dl, dr, ok, want_state, want_filled = check_reference(w, pattern)
    if pattern != "nan_negative":  # the pattern is what the judge sees
        assert np.array_equal(want_state == 0, np.broadcast_to(ok, want_state.shape))
    elif w >= 63:
        assert all((want_state == v).any() for v in (0, 1, 2))
    if pattern == "none":
        assert same_bits(want_filled, dl)
    lr = kernels.lr_check(torch.from_numpy(dl).to(DEV), torch.from_numpy(dr).to(DEV), 1.0)
    assert lr.state.dtype == torch.uint8 and lr.disp_filled.dtype == torch.float32
    assert np.array_equal(lr.state.cpu().numpy(), want_state)
    assert same_bits(lr.disp_filled.cpu().numpy(), want_filled)


@pytest.mark.parametrize("w", (1, 65, 1513))
def test_check_null_output_is_never_written(w):
    """Each output slot with a guard behind it, sentinel-filled; the slot whose pointer is
    passed as null and every guard keep the sentinel, the other slot holds the full call's
    values."""
    dl, dr, _, want_state, want_filled = check_reference(w, "nan_negative")
    n, guard = dl.size, 64
    tl, tr = torch.from_numpy(dl).to(DEV), torch.from_numpy(dr).to(DEV)
    lib = _lib.load()
    for want_s, want_f in ((True, True), (True, False), (False, True)):
        sbuf = torch.full((n + guard,), 77, dtype=torch.uint8, device=DEV)
        fbuf = torch.full((n + guard,), -12345.0, device=DEV)
        _lib.check(lib.lea_disparity_lr_check(tl.data_ptr(), tr.data_ptr(), sbuf.data_ptr() if want_s else None,
                                              fbuf.data_ptr() if want_f else None, LB, LH, w, 1.0,
                                              torch.cuda.current_stream().cuda_stream), "lea_disparity_lr_check")
        assert bool((sbuf[n:] == 77).all()) and bool((fbuf[n:] == -12345.0).all()), "a guard was written"
        if want_s:
            assert np.array_equal(sbuf[:n].cpu().numpy().reshape(dl.shape), want_state)
        else:
            assert bool((sbuf == 77).all()), "the null output's slot was written"
        if want_f:
            assert same_bits(fbuf[:n].cpu().numpy().reshape(dl.shape), want_filled)
        else:
            assert bool((fbuf == -12345.0).all()), "the null output's slot was written"
        part = kernels.lr_check(tl, tr, 1.0, want_s, want_f)
        assert (part.state is None) == (not want_s) and (part.disp_filled is None) == (not want_f)
    with pytest.raises(ValueError):
        kernels.lr_check(tl, tr, 1.0, False, False)


# ------------------------------------------------------------------ occlusion scene
def test_occlusion_scene_end_to_end():
    """A fronto-parallel foreground (disparity 30) over a background (9), with the band the
    foreground hides from the right camera left unmatched (constant cost): the plain head,
    the right head and the check flag the band and fill it with the background."""
    d3, h3, w3, md = 16, 8, 60, 48
    d = torch.full((h3, w3), 9.0)
    d[2:6, 25:40] = 30.0
    k = torch.arange(d3, dtype=torch.float32).view(d3, 1, 1)
    cost = 2 * (3 * k + 1 - d).abs()
    cost[:, 2:6, 18:25] = 20.0
    cost = cost.view(1, 1, d3, h3, w3)
    dev = cost.to(DEV)
    left = kernels.disparity_regression(dev, md)
    lr = kernels.lr_check(left, kernels.disparity_regression_right(dev, md), 1.0)
    state, filled = lr.state.cpu()[0, 8:16], lr.disp_filled.cpu()[0, 8:16]
    # the judge meets the same assertions (fp64 heads, the numpy check)
    u = F.interpolate(cost.double(), size=(md, 3 * h3, 3 * w3), mode="trilinear", align_corners=False)[:, 0]
    jl = (F.softmax(-u, dim=1) * torch.arange(md, dtype=torch.float64).view(1, md, 1, 1)).sum(1)
    js, jf = judge_check(jl.float().numpy(), judge_right(cost, torch.float64).float().numpy(), 1.0)
    for s, f in ((state.numpy(), filled.numpy()), (js[0, 8:16], jf[0, 8:16])):
        assert (s[:, 56:73] == 1).all()
        for lo, hi in ((12, 49), (78, 116), (125, 179)):
            assert (s[:, lo:hi + 1] == 0).all(), (lo, hi)
        assert (s[:, 0:9] == 2).all()
        assert (np.abs(f[:, 54:75] - 9) <= 0.5).all()


# ------------------------------------------------------------------ model level
H, W, MD = 96, 192, 48


def _model(precision="f32"):
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV, precision=precision)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def _pair(seed):
    return normal(seed, (1, 3, H, W)).to(DEV), normal(seed + 1, (1, 3, H, W)).to(DEV)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_forward_lr(precision):
    m = _model(precision)
    left, right = _pair(11)
    fast = precision == "bf16"
    with torch.no_grad():
        want = m(left, right)
        lr = m.forward_lr(left, right, 1.0)
        f = m.feature(left, right)
        cost = m.matching.executor().run_features(f[:1], f[1:], MD)
    assert isinstance(lr, kernels.DisparityLR)
    assert torch.equal(lr.disp, want)
    want_right = kernels.disparity_regression_right(cost, MD, fast)
    direct = kernels.lr_check(want, want_right, 1.0)
    assert torch.equal(lr.disp_right, want_right)
    assert torch.equal(lr.state, direct.state) and torch.equal(lr.disp_filled, direct.disp_filled)
    assert lr.state.dtype == torch.uint8 and set(lr.state.unique().tolist()) <= {0, 1, 2}
    good = lr.state == kernels.LR_CONSISTENT
    assert torch.equal(lr.disp_filled[good], lr.disp[good])
    assert torch.isfinite(lr.disp_right).all() and torch.isfinite(lr.disp_filled).all()


def test_forward_lr_is_inference_only():
    m = _model()
    left, right = _pair(11)
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_lr(left, right)
    m.eval()
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_lr(left.requires_grad_(), right)


def test_graphed_lr_replays_the_eager_call():
    m = _model()
    with pytest.raises(ValueError):
        m.graphed(1, H, W, confidence=True, lr_threshold=1.0)
    g = m.graphed(1, H, W, lr_threshold=1.0)
    for seed in (21, 31):
        left, right = _pair(seed)
        with torch.no_grad():
            want = m.forward_lr(left, right, 1.0)
        got = g(left, right)
        assert isinstance(got, kernels.DisparityLR)
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_predict_cli_lr_check(tmp_path):
    """The list of test_predict_cli_confidence, with and without --lr_check=1."""
    from PIL import Image
    from leastereo_amd import predict as P
    g = golden("c1_sceneflow")
    for side in ("left", "right"):
        d = tmp_path / "frames_finalpass" / "S" / side
        d.mkdir(parents=True)
        Image.fromarray(g[side + "_u8"][:96, :192]).save(d / "0001.png")
    (tmp_path / "list.txt").write_text("S/left/0001.png\n")
    torch.save({"state_dict": {"module." + k: v for k, v in state_dict().items()}}, tmp_path / "ckpt.pth")
    base = ["--sceneflow=1", f"--maxdisp={MD}", "--crop_height=96", "--crop_width=192",
            f"--data_path={tmp_path}/", f"--test_list={tmp_path}/list.txt", f"--resume={tmp_path}/ckpt.pth"]
    assert P.main(base + [f"--save_path={tmp_path}/plain/"]) == 0
    assert P.main(base + [f"--save_path={tmp_path}/lr/", "--lr_check=1"]) == 0
    new = ("0_right.npy", "0_occ.png", "0_filled.npy", "0_filled.png")
    for name in new:
        assert not (tmp_path / "plain" / name).exists() and (tmp_path / "lr" / name).exists(), name
    assert sorted(p.name for p in (tmp_path / "lr").iterdir()) == sorted(
        [p.name for p in (tmp_path / "plain").iterdir()] + list(new))
    assert np.array_equal(np.load(tmp_path / "plain" / "0.npy"), np.load(tmp_path / "lr" / "0.npy"))
    right, filled = np.load(tmp_path / "lr" / "0_right.npy"), np.load(tmp_path / "lr" / "0_filled.npy")
    assert right.shape == (96, 192) and right.dtype == np.float32
    assert filled.shape == (96, 192) and filled.dtype == np.float32
    occ = np.asarray(Image.open(tmp_path / "lr" / "0_occ.png"))
    assert occ.shape == (96, 192) and occ.dtype == np.uint8 and set(np.unique(occ).tolist()) <= {0, 127, 255}
    assert np.array_equal(filled[occ == 0], np.load(tmp_path / "lr" / "0.npy")[occ == 0])
    assert np.asarray(Image.open(tmp_path / "lr" / "0_filled.png")).shape[:2] == (96, 192)
    # together with --confidence: both sets of files, the same disparity
    assert P.main(base + [f"--save_path={tmp_path}/both/", "--lr_check=1", "--confidence=peak"]) == 0
    for name in new + ("0_conf.npy", "0_conf.png", "0_local.npy"):
        assert (tmp_path / "both" / name).exists(), name
    assert np.array_equal(np.load(tmp_path / "plain" / "0.npy"), np.load(tmp_path / "both" / "0.npy"))
    assert np.array_equal(np.load(tmp_path / "both" / "0_right.npy"), right)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "both" / "0_occ.png")), occ)


def test_predict_cli_satellite_lr_check(tmp_path):
    """The satellite loop with --lr_check=1: <name>_occ.png beside <name>.png, the state map of
    forward_lr as 0 / 127 / 255 cropped like the disparity (a 90 x 180 input padded into the
    96 x 192 crop); <name>.png is what it is without the flag."""
    from PIL import Image
    from leastereo_amd import predict as P
    g = golden("c1_sceneflow")
    d = tmp_path / "sat" / "tile_01"
    d.mkdir(parents=True)
    Image.fromarray(g["left_u8"][:90, :180]).save(d / "satiml.png")
    Image.fromarray(g["right_u8"][:90, :180]).save(d / "satimr.png")
    (tmp_path / "list.txt").write_text("tile_01\n")
    torch.save({"state_dict": state_dict()}, tmp_path / "ckpt.pth")
    base = ["--satellite=1", f"--maxdisp={MD}", "--crop_height=96", "--crop_width=192", f"--data_path={tmp_path}/sat/",
            f"--test_list={tmp_path}/list.txt", f"--resume={tmp_path}/ckpt.pth"]
    for name, extra in (("plain", []), ("lr", ["--lr_check=1"])):
        (tmp_path / name).mkdir()
        assert P.main(base + [f"--save_path={tmp_path}/{name}/"] + extra) == 0
    assert not (tmp_path / "plain" / "tile_01_occ.png").exists()
    for name in ("tile_01.png", "tile_01_in.png"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "lr" / name).read_bytes(), name
    left, right, h, w = P.load_transform(*P.load_images(d / "satiml.png", d / "satimr.png"), 96, 192)
    with torch.no_grad():
        lr = _model().forward_lr(left, right, 1.0)
    want = P.occlusion_u8(P.crop_output(lr.state.cpu().numpy(), h, w, 96, 192))
    got = np.asarray(Image.open(tmp_path / "lr" / "tile_01_occ.png"))
    assert got.shape == (90, 180) and got.dtype == np.uint8 and np.array_equal(got, want)
