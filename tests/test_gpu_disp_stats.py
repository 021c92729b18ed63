"""The confidence head (lea_disparity_regression_stats) on the GPU against an fp64 judge.

The judge is written here: Disp (models/build_model_2d.py:52-57) restated in torch --
trilinear align_corners=False up-sampling of the cost to U [MD, 3H3, 3W3] and to the
planes v [D3, 3H3, 3W3], log_softmax(-U) -- plus the definitions of the header:
entropy = -sum p ln p, winner od* = 3 argmin_k v[k] + 1, peak = the mass within r of it,
disp_local = that window's soft-argmin.

Bars (none taken from what the kernel gives): for entropy, peak and disp_local the max abs
error against fp64 is at most max(4 x E_cpu, 32 ulp of the output's range), E_cpu being the
same restatement run in float32 on the CPU for that very case (ranges ln MD, 1, MD; the 4
covers the other summation order and the factored form's three rounded exponentials per
term).  The hardware-exp dtype gets the same bar times R = max(1, err(plain fast disp) /
err(plain f32 disp)), both of the existing entry against fp64 on that case.  Pixels whose
two smallest planes differ by less than 1e-4 x scale in fp64 (the winner may legitimately
differ) are left out of the peak / disp_local comparison; at most 0.2 % of a case's pixels.
Each case prints its figures before it asserts (pytest -s).
"""
import functools
import itertools
import math

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
SHAPES = [(2, 4, 5, 7),      # three-row form; odd sizes: every clamp edge; batch stride
          (1, 8, 3, 90),     # Wo = 270 > 256: two workgroups along W, the second partial, c_lo > 0
          (1, 64, 4, 90),    # the product depth
          (1, 88, 3, 90),    # the two-row form of C5
          (2, 5, 4, 6)]      # unconfigured depth: the generic form
CONFIGURED = (4, 8, 16, 32, 64, 88)
SCALES = (1, 3, 20)          # flat to sharp
TIE = 1e-4                   # near-tie gap, x scale
TIE_CAP = 0.002


def make_cost(shape, scale):
    b, d3, h3, w3 = shape
    g = torch.Generator().manual_seed(0)
    return torch.randn(b, 1, d3, h3, w3, generator=g) * scale


def judge_base(cost, dtype):
    """U -> p, log p, the planes v (torch CPU, ``dtype``)."""
    x = cost.to(dtype)
    _, _, d3, h3, w3 = x.shape
    md = 3 * d3
    u = F.interpolate(x, size=(md, 3 * h3, 3 * w3), mode="trilinear", align_corners=False)[:, 0]
    v = F.interpolate(x, size=(d3, 3 * h3, 3 * w3), mode="trilinear", align_corners=False)[:, 0]
    logp = F.log_softmax(-u, dim=1)
    p = logp.exp()
    od = torch.arange(md, dtype=dtype).view(1, md, 1, 1)
    disp = (p * od).sum(1)
    entropy = -torch.where(p > 0, p * logp, torch.zeros_like(p)).sum(1)
    two = v.topk(2, dim=1, largest=False).values if d3 > 1 else torch.stack((v[:, 0], v[:, 0] + 1), 1)
    return dict(p=p, od=od, disp=disp, entropy=entropy, ods=3 * v.argmin(1) + 1, gap=two[:, 1] - two[:, 0])


def judge_window(base, r):
    win = ((base["od"] - base["ods"].unsqueeze(1).to(base["od"].dtype)).abs() <= r).to(base["p"].dtype)
    peak = (base["p"] * win).sum(1)
    return peak, (base["p"] * win * base["od"]).sum(1) / peak


@functools.lru_cache(None)
def reference(shape, scale):
    """Per (shape, scale), computed once and left unchanged: the cost, the fp64 judge, its
    float32 restatement, the near-tie mask and the plain entry's two errors against fp64."""
    cost = make_cost(shape, scale)
    j64, j32 = judge_base(cost, torch.float64), judge_base(cost, torch.float32)
    keep = j64["gap"] >= TIE * scale
    # the float32 restatement must have the judge's winner wherever the pixel is compared
    assert torch.equal(j64["ods"][keep], j32["ods"][keep])
    dev = cost.to(DEV)
    md = 3 * shape[1]
    plain = {fast: kernels.disparity_regression(dev, md, fast).cpu() for fast in (False, True)}
    err = {fast: float((plain[fast].double() - j64["disp"]).abs().max()) for fast in (False, True)}
    return dict(cost=dev, j64=j64, j32=j32, keep=keep, plain=plain, R=max(1.0, err[True] / err[False]),
                plain_err=err)


def ulp_of(x):
    return float(np.spacing(np.float32(x)))


def check_case(shape, scale, fast, r):
    ref = reference(shape, scale)
    md = 3 * shape[1]
    st = kernels.disparity_regression_stats(ref["cost"], md, r, fast)
    got = {k: getattr(st, k).cpu() for k in ("disp", "entropy", "peak", "disp_local")}
    keep = ref["keep"]
    dropped = 1.0 - float(keep.double().mean())
    p64, l64 = judge_window(ref["j64"], r)
    p32, l32 = judge_window(ref["j32"], r)
    want = dict(disp=ref["j64"]["disp"], entropy=ref["j64"]["entropy"], peak=p64, disp_local=l64)
    cpu32 = dict(disp=ref["j32"]["disp"], entropy=ref["j32"]["entropy"], peak=p32, disp_local=l32)
    span = dict(disp=md, entropy=math.log(md), peak=1.0, disp_local=md)
    R = ref["R"] if fast else 1.0
    fails = []
    for k in ("disp", "entropy", "peak", "disp_local"):
        sel = keep if k in ("peak", "disp_local") else torch.ones_like(keep)
        e_cpu = float((cpu32[k].double() - want[k])[sel].abs().max())
        e_gpu = float((got[k].double() - want[k])[sel].abs().max())
        bar = max(4 * e_cpu, 32 * ulp_of(span[k])) * R
        print(f"{shape} x{scale} fast={int(fast)} r={r} {k:10s} gpu {e_gpu:.3e} cpu32 {e_cpu:.3e} "
              f"bar {bar:.3e} R {R:.2f} gpu/cpu32 {e_gpu / max(e_cpu, 1e-30):.2f} dropped {dropped:.5f}")
        assert torch.isfinite(got[k]).all(), k
        if k == "disp" and shape[1] in CONFIGURED:
            continue  # judged by bit-identity below
        if not e_gpu <= bar:
            fails.append((k, e_gpu, bar))
    assert dropped <= TIE_CAP, dropped
    if shape[1] in CONFIGURED:
        assert torch.equal(got["disp"], ref["plain"][fast]), "disp differs from lea_disparity_regression"
    assert not fails, fails
    assert float(got["entropy"].min()) >= 0 and float(got["entropy"].max()) <= math.log(md) * (1 + 1e-6)
    assert float(got["peak"].min()) > 0 and float(got["peak"].max()) <= 1


@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("fast", [False, True], ids=["f32", "hwexp"])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stats_against_fp64(shape, scale, fast, r):
    check_case(shape, scale, fast, r)


@pytest.mark.parametrize("fast", [False, True], ids=["f32", "hwexp"])
def test_radius_16_covers_everything_at_d3_4(fast):
    """MD = 12: every od lies within 16 of the winner, so peak = 1 and disp_local = disp."""
    check_case((2, 4, 5, 7), 3, fast, 16)
    ref = reference((2, 4, 5, 7), 3)
    st = kernels.disparity_regression_stats(ref["cost"], 12, 16, fast)
    assert float((st.peak - 1).abs().max()) <= 2 ** -22
    assert float((st.disp_local - st.disp).abs().max()) <= 32 * ulp_of(12)


@pytest.mark.parametrize("fast", [False, True], ids=["f32", "hwexp"])
@pytest.mark.parametrize("shape", [(1, 16, 3, 5), (1, 32, 3, 5)], ids=lambda s: "x".join(map(str, s)))
def test_disp_bit_identity_at_the_other_configured_depths(shape, fast):
    """(16, 48) and (32, 96): with the four configured shapes above, every configured depth."""
    cost = make_cost(shape, 3).to(DEV)
    md = 3 * shape[1]
    assert torch.equal(kernels.disparity_regression_stats(cost, md, 4, fast).disp,
                       kernels.disparity_regression(cost, md, fast))


# ------------------------------------------------------------------ analytic cases
@pytest.mark.parametrize("fast", [False, True], ids=["f32", "hwexp"])
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_constant_cost(shape, r, fast):
    """Every exponential is 1: entropy = ln MD, the winner is plane 0 (od* = 1), the window
    [0, r + 1] holds r + 2 samples: peak = (r + 2) / MD, disp_local = (r + 1) / 2."""
    b, d3, h3, w3 = shape
    md = 3 * d3
    st = kernels.disparity_regression_stats(torch.full((b, 1, d3, h3, w3), 0.7, device=DEV), md, r, fast)
    assert float((st.entropy - math.log(md)).abs().max()) <= 4 * ulp_of(math.log(md))
    assert torch.equal(st.peak, torch.full_like(st.peak, (r + 2) / md))
    assert torch.equal(st.disp_local, torch.full_like(st.peak, (r + 1) / 2))
    assert torch.equal(st.disp, torch.full_like(st.peak, (md - 1) / 2))


@pytest.mark.parametrize("fast", [False, True], ids=["f32", "hwexp"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_plane_far_below_the_rest(shape, fast):
    """Plane k lower by G = 300: the neighbours' e^-100 and the rest's e^-300 underflow; no
    NaN / Inf may come of the underflowed terms.  An interior k: entropy -> 0, peak -> 1,
    disp_local -> 3k + 1.  The first and last plane own two equal samples (U[0] == U[1],
    U[MD-2] == U[MD-1]: the clamped ends): entropy -> ln 2, disp_local -> 0.5 and MD - 1.5."""
    b, d3, h3, w3 = shape
    md = 3 * d3
    for k in sorted({0, 1, d3 // 2, d3 - 2, d3 - 1}):
        cost = torch.zeros(b, 1, d3, h3, w3, device=DEV)
        cost[:, :, k] = -300.0
        st = kernels.disparity_regression_stats(cost, md, 4, fast)
        for t in st:
            assert torch.isfinite(t).all()
        end = k in (0, d3 - 1)
        want_h = math.log(2) if end else 0.0
        want_d = 0.5 if k == 0 else (md - 1.5 if k == d3 - 1 else 3 * k + 1)
        assert float((st.entropy - want_h).abs().max()) <= (4 * ulp_of(want_h) if end else 1e-30)
        assert float(st.entropy.min()) >= 0
        assert torch.equal(st.peak, torch.ones_like(st.peak))
        assert float((st.disp_local - want_d).abs().max()) <= 4 * ulp_of(md)
        assert float((st.disp - want_d).abs().max()) <= 4 * ulp_of(md)


# ------------------------------------------------------------------ optional outputs
@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (1, 88, 3, 90), (2, 5, 4, 6)], ids=lambda s: "x".join(map(str, s)))
def test_each_subset_gives_the_full_call_values(shape):
    ref = reference(shape, 3)
    md = 3 * shape[1]
    full = kernels.disparity_regression_stats(ref["cost"], md, 4)
    for want in itertools.product((False, True), repeat=3):
        if not any(want):
            with pytest.raises(ValueError):
                kernels.disparity_regression_stats(ref["cost"], md, 4, False, *want)
            continue
        part = kernels.disparity_regression_stats(ref["cost"], md, 4, False, *want)
        assert torch.equal(part.disp, full.disp)
        for asked, a, f in zip(want, part[1:], full[1:]):
            assert (a is None) == (not asked)
            if asked:
                assert torch.equal(a, f)


@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (1, 88, 3, 90), (2, 5, 4, 6)], ids=lambda s: "x".join(map(str, s)))
def test_null_output_is_never_written(shape):
    """Four output slots with guards between them in ONE allocation, sentinel-filled; the
    slot whose pointer is passed as null and every guard keep the sentinel."""
    ref = reference(shape, 3)
    b, d3, h3, w3 = shape
    n, guard, sentinel = b * 9 * h3 * w3, 64, -12345.0
    full = kernels.disparity_regression_stats(ref["cost"], 3 * d3, 4)
    lib = _lib.load()
    for hole in (1, 2, 3):
        buf = torch.full((4, n + guard), sentinel, device=DEV)
        ptr = [None if i == hole else buf[i].data_ptr() for i in range(4)]
        _lib.check(lib.lea_disparity_regression_stats(ref["cost"].data_ptr(), *ptr, b, d3, h3, w3, 3 * d3, 4,
                                                      _lib.LEA_F32, torch.cuda.current_stream().cuda_stream),
                   "lea_disparity_regression_stats")
        assert bool((buf[:, n:] == sentinel).all()), "a guard was written"
        assert bool((buf[hole] == sentinel).all()), "the null output's slot was written"
        for i in range(4):
            if i != hole:
                assert torch.equal(buf[i, :n].view(b, 3 * h3, 3 * w3), full[i])


def test_refusals_reach_python():
    cost = torch.zeros(1, 1, 4, 2, 2, device=DEV)
    with pytest.raises(_lib.HipKernelError, match="maxdisp"):
        kernels.disparity_regression_stats(cost, 13)
    with pytest.raises(_lib.HipKernelError, match="radius"):
        kernels.disparity_regression_stats(cost, 12, radius=17)


# ------------------------------------------------------------------ model level
H, W, MD = 96, 192, 48


def _model(precision="f32"):
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV, precision=precision)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def _pair(seed):
    return normal(seed, (1, 3, H, W)).to(DEV), normal(seed + 1, (1, 3, H, W)).to(DEV)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_forward_with_confidence(precision):
    m = _model(precision)
    left, right = _pair(11)
    r = 4
    with torch.no_grad():
        want = m(left, right)
        st = m.forward_with_confidence(left, right, r)
        # the matching cost the head saw, for the winner (forward's own steps)
        f = m.feature(left, right)
        cost = m.matching.executor().run_features(f[:1], f[1:], MD)
    assert torch.equal(st.disp, want)
    assert st.maxdisp == MD and st.entropy.shape == want.shape
    assert float(st.entropy.min()) >= 0 and float(st.entropy.max()) <= math.log(MD) * (1 + 1e-6)
    assert float(st.peak.min()) > 0 and float(st.peak.max()) <= 1
    conf = st.confidence
    assert float(conf.min()) >= -1e-6 and float(conf.max()) <= 1
    # |disp_local - od*| <= r, od* from the fp64 planes of that cost; at a near-tie the winner
    # may be the runner-up plane instead (a real network's cost has flat regions: no cap here)
    x = cost.cpu().double()
    v = F.interpolate(x, size=(MD // 3, H, W), mode="trilinear", align_corners=False)[:, 0]
    val, idx = v.topk(2, dim=1, largest=False)
    near = (val[:, 1] - val[:, 0]) < TIE * float(x.abs().max())
    local = st.disp_local.cpu().double()
    first, second = ((local - (3 * idx[:, i] + 1)).abs() <= r for i in (0, 1))
    assert bool((first | (near & second)).all())


def test_forward_with_confidence_is_inference_only():
    m = _model()
    left, right = _pair(11)
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_with_confidence(left, right)
    m.eval()
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_with_confidence(left.requires_grad_(), right)


def test_graphed_confidence_replays_the_eager_call():
    m = _model()
    g = m.graphed(1, H, W, confidence=True, radius=4)
    for seed in (21, 31):
        left, right = _pair(seed)
        with torch.no_grad():
            want = m.forward_with_confidence(left, right, 4)
        got = g(left, right)
        assert isinstance(got, kernels.DisparityStats) and got.maxdisp == MD
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_predict_cli_confidence(tmp_path):
    """The list of test_predict_cli_runs_on_a_list, with and without --confidence=peak."""
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
    assert P.main(base + [f"--save_path={tmp_path}/conf/", "--confidence=peak"]) == 0
    assert not (tmp_path / "plain" / "0_conf.npy").exists() and not (tmp_path / "plain" / "0_local.npy").exists()
    assert np.array_equal(np.load(tmp_path / "plain" / "0.npy"), np.load(tmp_path / "conf" / "0.npy"))
    conf, local = np.load(tmp_path / "conf" / "0_conf.npy"), np.load(tmp_path / "conf" / "0_local.npy")
    assert conf.shape == (96, 192) and conf.dtype == np.float32 and conf.min() > 0 and conf.max() <= 1
    assert local.shape == (96, 192) and local.dtype == np.float32 and local.min() >= 0 and local.max() <= MD - 1
    png = np.asarray(Image.open(tmp_path / "conf" / "0_conf.png"))
    assert png.shape == (96, 192) and png.dtype == np.uint8


def test_predict_cli_satellite_confidence(tmp_path):
    """The satellite loop with --confidence=entropy: <name>_conf.png beside <name>.png, the
    8-bit image of DisparityStats.confidence cropped like the disparity (a 90 x 180 input
    padded into the 96 x 192 crop), and no _local file."""
    from PIL import Image
    from leastereo_amd import predict as P
    g = golden("c1_sceneflow")
    d = tmp_path / "sat" / "tile_01"
    d.mkdir(parents=True)
    Image.fromarray(g["left_u8"][:90, :180]).save(d / "satiml.png")
    Image.fromarray(g["right_u8"][:90, :180]).save(d / "satimr.png")
    (tmp_path / "list.txt").write_text("tile_01\n")
    out = tmp_path / "out"
    out.mkdir()
    torch.save({"state_dict": state_dict()}, tmp_path / "ckpt.pth")
    assert P.main(["--satellite=1", f"--maxdisp={MD}", "--crop_height=96", "--crop_width=192",
                   f"--data_path={tmp_path}/sat/", f"--test_list={tmp_path}/list.txt", f"--save_path={out}/",
                   f"--resume={tmp_path}/ckpt.pth", "--confidence=entropy"]) == 0
    left, right, h, w = P.load_transform(*P.load_images(d / "satiml.png", d / "satimr.png"), 96, 192)
    with torch.no_grad():
        st = _model().forward_with_confidence(left, right)
    want = P.float_to_u8(np.clip(P.crop_output(st.confidence.cpu().numpy(), h, w, 96, 192), 0.0, 1.0))
    got = np.asarray(Image.open(out / "tile_01_conf.png"))
    assert got.shape == (90, 180) and np.array_equal(got, want)
    assert np.asarray(Image.open(out / "tile_01.png")).shape == (90, 180)
    assert not list(out.glob("*_local*"))
