"""Photometric consistency on the GPU: lea_photometric_f32 and lea_photometric_grad_f32
through kernels.photometric_sums / photometric_grad and losses.photometric_loss.

The judge is the definition in torch on the CPU (tests/photo_judge.py), in float64; the bar
is the project's convention (test_gpu_loss.py, test_gpu_lr.py): an error against fp64 of at
most max(4 x E_cpu32, 8 ulp_f32 of the quantity), E_cpu32 being the same judge run in
float32 on the CPU for that very case; for the per-pixel gradient the quantity is the
largest gradient of the case.  Counts are exact, the warped image is within 2 ulp of the
fp64 value pixel by pixel, and err is -1 exactly where v fails.

Shapes are the smallest that reach each path: one window; a small multi-channel batch; a
case that crosses the 64 x 16 tile (kPhW, kPhH in csrc/photometric.hip) with padded batch
strides; and the tile plus one row and one column with four channels.
"""
import functools

import numpy as np
import pytest
import torch

from leastereo_amd import kernels, losses
from tests import photo_judge
from tests.photo_judge import ALPHA

pytestmark = pytest.mark.gpu
DEV = "cuda"

TILE_W, TILE_H = 64, 16
SHAPES = [(1, 1, 3, 3), (2, 3, 5, 8), (2, 3, 17, 70), (1, 4, TILE_H + 1, TILE_W + 1)]
PADDED = (2, 3, 17, 70)
CASES = [(s, k) for k in ("grid", "float", "exclude") for s in SHAPES] + [(PADDED, "smooth")]
IDS = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)


def padded(t):
    """The tensor on the device with a batch stride 11 elements larger than its block, as
    to_device(..., padded_batch_stride=True) of test_gpu_loss.py."""
    b, n = t.shape[0], t[0].numel()
    buf = torch.full((b, n + 11), 77, device=DEV, dtype=t.dtype)
    buf[:, :n] = t.reshape(b, -1).to(DEV)
    v = buf[:, :n].view(t.shape)
    assert v.stride(0) == n + 11
    return v


@functools.lru_cache(None)
def device_case(shape, kind):
    left, right, disp, exclude = photo_judge.make_case(shape, kind)
    put = padded if shape == PADDED else (lambda t: t.to(DEV))
    return put(left), put(right), put(disp), None if exclude is None else put(exclude)


def ulp_of(x):
    return float(np.spacing(np.float32(abs(x))))


def run_entries(shape, kind, scales=(1 - ALPHA, ALPHA), maps=False):
    left, right, disp, exclude = device_case(shape, kind)
    out = kernels.photometric_sums(left, right, disp, exclude, ALPHA, want_warped=maps, want_err=maps)
    sums = out[0] if maps else out
    grad = kernels.photometric_grad(left, right, disp, exclude, sums=sums,
                                    scales=torch.tensor(scales, device=DEV, dtype=torch.float32))
    return (sums, grad) + (tuple(out[1:]) if maps else ())


@pytest.mark.parametrize("shape,kind", CASES, **IDS)
def test_sums_maps_and_gradient_against_fp64(shape, kind):
    b, c, h, w = shape
    j64, j32 = photo_judge.judged(shape, kind), photo_judge.judged(shape, kind, torch.float32)
    sums, grad, warped, err = run_entries(shape, kind, maps=True)
    assert sums.dtype == torch.float64 and sums.is_cuda and sums.shape == (4,)
    assert grad.shape == (b, h, w) and grad.dtype == torch.float32
    assert warped.shape == shape and err.shape == (b, h, w)
    s = sums.cpu().tolist()
    print(f"{shape} {kind}: n_view {s[0]:.0f} of {b * h * w}, n_window {s[2]:.0f} of {b * (h - 2) * (w - 2)}")
    assert s[0] == j64["n_view"] and s[2] == j64["n_window"], "the counts are exact"
    if shape == (1, 1, 3, 3):
        assert s[0] == 9 and s[2] == 1
    elif kind != "exclude":
        assert 0 < s[0] < b * h * w and 0 < s[2] < b * (h - 2) * (w - 2), "both masks bite"
    else:
        assert 0 < s[0] < int(j64["in_view"].sum()) and s[2] > 0, "the exclusion bites and windows survive"
    l1, dssim = s[1] / s[0], (s[3] / s[2] if s[2] else 0.0)
    loss = (1 - ALPHA) * l1 + ALPHA * dssim
    fails = []
    for name, got in (("l1", l1), ("dssim", dssim), ("loss", loss)):
        want, cpu32 = j64[name], j32[name]
        e_gpu, e_cpu = abs(got - want), abs(cpu32 - want)
        bar = max(4 * e_cpu, 8 * ulp_of(want))
        print(f"{shape} {kind} {name}: fp64 {want:.9g} gpu err {e_gpu:.3e} cpu32 err {e_cpu:.3e} bar {bar:.3e}")
        if not e_gpu <= bar:
            fails.append((name, e_gpu, bar))
    g64, g32 = j64["ddisp"], j32["ddisp"]
    gmax = float(g64.abs().max())
    e_gpu = float((grad.cpu().double() - g64).abs().max())      # every pixel
    e_cpu = float((g32.double() - g64).abs().max())
    bar = max(4 * e_cpu, 8 * ulp_of(gmax))
    print(f"{shape} {kind} ddisp: max |g| {gmax:.6g} gpu err {e_gpu:.3e} cpu32 err {e_cpu:.3e} bar {bar:.3e}")
    assert torch.isfinite(grad).all()
    if not e_gpu <= bar:
        fails.append(("ddisp", e_gpu, bar))
    assert bool((grad.cpu()[~j64["v"]] == 0).all()), "no gradient where v fails"
    # the maps
    w64 = j64["warped"].numpy()
    werr = np.abs(warped.cpu().numpy().astype(np.float64) - w64)
    wulp = np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64)
    print(f"{shape} {kind} warped: worst error {float((werr / wulp).max()):.3f} ulp")
    if not bool((werr <= 2 * wulp).all()):
        fails.append(("warped", float((werr / wulp).max()), 2.0))
    out_of_view = ~j64["in_view"].unsqueeze(1).expand(shape)
    assert bool((warped.cpu()[out_of_view] == 0).all())
    e = err.cpu()
    assert bool((e[~j64["v"]] == -1).all()) and bool((e[j64["v"]] >= 0).all()), "err is -1 exactly where v fails"
    e_gpu = float((e.double() - j64["err"])[j64["v"]].abs().max())
    e_cpu = float((j32["err"].double() - j64["err"])[j64["v"]].abs().max())
    bar = max(4 * e_cpu, 8 * ulp_of(float(j64["err"].max())))
    print(f"{shape} {kind} err map: gpu err {e_gpu:.3e} cpu32 err {e_cpu:.3e} bar {bar:.3e}")
    if not e_gpu <= bar:
        fails.append(("err", e_gpu, bar))
    assert not fails, fails


@pytest.mark.parametrize("scales", [(1.0, 0.0), (0.0, 1.0)], ids=["l1", "dssim"])
def test_each_part_of_the_gradient(scales):
    shape = PADDED
    left, right, disp, exclude = photo_judge.make_case(shape, "grid")
    g64 = photo_judge.judge(left, right, disp, exclude, scales=scales)["ddisp"]
    g32 = photo_judge.judge(left, right, disp, exclude, scales=scales, dtype=torch.float32)["ddisp"]
    _, grad = run_entries(shape, "grid", scales=scales)
    e_gpu = float((grad.cpu().double() - g64).abs().max())
    e_cpu = float((g32.double() - g64).abs().max())
    bar = max(4 * e_cpu, 8 * ulp_of(float(g64.abs().max())))
    print(f"scales {scales}: gpu err {e_gpu:.3e} cpu32 err {e_cpu:.3e} bar {bar:.3e}")
    assert e_gpu <= bar


# ------------------------------------------------------------------ structural cases

def shifted_pair(shape, k):
    """left[x] = right[x - k]; the k leftmost columns of left are fresh noise."""
    gen = torch.Generator().manual_seed(3)
    right = torch.randn(shape, generator=gen)
    left = torch.randn(shape, generator=gen)
    left[..., k:] = right[..., : shape[3] - k]
    return left.to(DEV), right.to(DEV)


def test_exact_shift_has_zero_l1():
    shape, k = (2, 3, 17, 70), 3
    b, c, h, w = shape
    left, right = shifted_pair(shape, k)
    disp = torch.full((b, h, w), float(k), device=DEV)
    sums = kernels.photometric_sums(left, right, disp)
    s = sums.cpu().tolist()
    assert s[0] == b * h * (w - k) and s[2] == b * (h - 2) * (w - k - 2)
    assert s[1] == 0, "w == left exactly on every pixel in view"
    assert s[3] >= 0
    g_l1 = kernels.photometric_grad(left, right, disp, sums=sums, scales=torch.tensor([1.0, 0.0], device=DEV))
    assert bool((g_l1 == 0).all()), "sign(0) = 0"
    # the other sign of the disparity is another image: this catches the convention
    s_neg = kernels.photometric_sums(left, right, -disp).cpu().tolist()
    assert s_neg[0] == b * h * (w - k) and s_neg[1] > 0


@pytest.mark.parametrize("how", ["out_of_view", "excluded"])
def test_no_pixel_takes_part(how):
    shape = (2, 3, 17, 70)
    b, c, h, w = shape
    left, right, disp, _ = device_case(shape, "grid")
    exclude = None
    if how == "out_of_view":
        disp = torch.full((b, h, w), float(w + 1), device=DEV)
    else:
        exclude = torch.full((b, h, w), 2, device=DEV, dtype=torch.uint8)
    sums, warped, err = kernels.photometric_sums(left, right, disp, exclude, want_warped=True, want_err=True)
    assert sums.cpu().tolist() == [0, 0, 0, 0]
    assert bool((err == -1).all())
    if how == "out_of_view":
        assert bool((warped == 0).all())
    grad = kernels.photometric_grad(left, right, disp, exclude, sums=sums,
                                    scales=torch.tensor([1 - ALPHA, ALPHA], device=DEV))
    assert torch.isfinite(grad).all() and bool((grad == 0).all())
    # the wrapper: 0, not NaN
    d = disp.clone().requires_grad_()
    loss, (l1, dssim, n_v, n_w) = losses.photometric_loss(left, right, d, exclude, return_parts=True)
    loss.backward()
    assert all(float(t.detach()) == 0 for t in (loss, l1, dssim, n_v, n_w))
    assert bool((d.grad == 0).all())


def test_bool_exclude_and_lr_state_values():
    """Any non-zero byte excludes (the left-right check's states 1 and 2), and a bool mask is
    taken as it is."""
    shape = (2, 3, 17, 70)
    left, right, disp, exclude = device_case(shape, "exclude")
    want = kernels.photometric_sums(left, right, disp, exclude)
    twos = exclude * 2
    assert torch.equal(kernels.photometric_sums(left, right, disp, twos), want)
    assert torch.equal(kernels.photometric_sums(left, right, disp, exclude.bool()), want)


# ------------------------------------------------------------------ determinism, capture

def test_two_runs_give_identical_bits():
    a = run_entries(PADDED, "grid", maps=True)
    b = run_entries(PADDED, "grid", maps=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_graph_capture_replays_the_eager_calls():
    """A capture cannot contain a host synchronisation or a read-back: this is also the
    test that neither entry does either."""
    shape = (2, 3, 17, 70)
    first = [t.to(DEV) for t in photo_judge.make_case(shape, "grid")[:3]]
    second = [t.to(DEV) for t in photo_judge.make_case(shape, "float")[:3]]
    left, right, disp = (t.clone() for t in first)
    scales = torch.tensor([1 - ALPHA, ALPHA], device=DEV)

    def step(l, r, d):
        sums = kernels.photometric_sums(l, r, d, None, ALPHA)
        return sums, kernels.photometric_grad(l, r, d, sums=sums, scales=scales)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(left, right, disp)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(left, right, disp)
    for case in (second, first):
        for dst, src in zip((left, right, disp), case):
            dst.copy_(src)
        graph.replay()
        want = step(*case)
        for got, w in zip(out, want):
            assert torch.equal(got.view(torch.uint8), w.view(torch.uint8))
    assert not torch.equal(step(*first)[1], step(*second)[1])


# ------------------------------------------------------------------ the autograd wrapper

def test_photometric_loss_backward_is_the_grad_entry():
    shape = (2, 3, 17, 70)
    left, right, disp, exclude = device_case(shape, "exclude")
    sums, want = run_entries(shape, "exclude")
    d = disp.clone().requires_grad_()
    lf, rt = left.clone().requires_grad_(), right.clone().requires_grad_()
    loss, parts = losses.photometric_loss(lf, rt, d, exclude, return_parts=True)
    for t in (loss,) + parts:
        assert t.is_cuda and t.dim() == 0
    loss.backward()
    assert torch.equal(d.grad, want) and lf.grad is None and rt.grad is None
    s = sums.cpu().tolist()
    l1, dssim, n_v, n_w = parts
    assert float(n_v) == s[0] and float(n_w) == s[2]
    assert float(l1) == pytest.approx(s[1] / s[0], rel=1e-6) and float(dssim) == pytest.approx(s[3] / s[2], rel=1e-6)
    assert float(loss) == pytest.approx(photo_judge.judged(shape, "exclude")["loss"], rel=1e-5)
    # the plain call returns the loss alone; [B, 1, H, W] disparities are taken as combined_loss takes them
    d4 = disp.unsqueeze(1).clone().requires_grad_()
    again = losses.photometric_loss(left, right, d4, exclude)
    assert torch.equal(again.detach(), loss.detach())
    again.backward()
    assert d4.grad.shape == (2, 1, 17, 70) and torch.equal(d4.grad.squeeze(1), want)
    # the parts carry their own gradients: d l1 alone is the (1, 0) gradient
    d1 = disp.clone().requires_grad_()
    losses.photometric_loss(left, right, d1, exclude, return_parts=True)[1][0].backward()
    assert torch.equal(d1.grad, run_entries(shape, "exclude", scales=(1.0, 0.0))[1])


def test_whole_model_step_with_the_photometric_term():
    """model.train(), masked smooth-L1 + 0.1 x photometric loss, backward: every parameter
    gradient is finite and differs from the plain loss's (96 x 192 D48, the smallest
    training shape of test_gpu_training.py)."""
    from leastereo_amd.config import LEAStereoArgs, default_arch_args
    from leastereo_amd.model import LEAStereo
    from leastereo_amd.weights import seeded_normal
    from tests.golden_util import state_dict
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=48)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    m = m.to(DEV).train()
    left = torch.from_numpy(seeded_normal(311, (1, 3, 96, 192))).to(DEV)
    right = torch.from_numpy(seeded_normal(312, (1, 3, 96, 192))).to(DEV)
    target = torch.from_numpy(seeded_normal(313, (1, 96, 192))).to(DEV) * 4 + 20

    def grads(photo_w):
        m.zero_grad(set_to_none=True)
        disp = m(left, right)
        loss = losses.masked_smooth_l1(disp, target, 48.0)
        if photo_w:
            photo, (_, _, n_v, n_w) = losses.photometric_loss(left, right, disp, return_parts=True)
            assert float(n_v) > 0 and float(n_w) > 0 and float(photo) > 0
            loss = loss + photo_w * photo
        loss.backward()
        # parameters the genotype leaves unused get no gradient from either loss
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    plain, both = grads(0.0), grads(0.1)
    assert sorted(plain) == sorted(both) and len(plain) > 300
    for k, g in both.items():
        assert torch.isfinite(g).all(), k
        assert not torch.equal(g, plain[k]), k


def test_predict_cli_photo_check(tmp_path, capsys):
    """The list of test_predict_cli_lr_check, with and without --photo_check, and with both."""
    from PIL import Image
    from leastereo_amd import predict as P
    from tests.golden_util import golden, state_dict
    g = golden("c1_sceneflow")
    for side in ("left", "right"):
        d = tmp_path / "frames_finalpass" / "S" / side
        d.mkdir(parents=True)
        Image.fromarray(g[side + "_u8"][:96, :192]).save(d / "0001.png")
    (tmp_path / "list.txt").write_text("S/left/0001.png\n")
    torch.save({"state_dict": {"module." + k: v for k, v in state_dict().items()}}, tmp_path / "ckpt.pth")
    base = ["--sceneflow=1", "--maxdisp=48", "--crop_height=96", "--crop_width=192",
            f"--data_path={tmp_path}/", f"--test_list={tmp_path}/list.txt", f"--resume={tmp_path}/ckpt.pth"]
    assert P.main(base + [f"--save_path={tmp_path}/plain/"]) == 0
    assert "photometric" not in capsys.readouterr().out
    assert P.main(base + [f"--save_path={tmp_path}/photo/", "--photo_check"]) == 0
    assert "0: mean photometric error" in capsys.readouterr().out
    new = ("0_warped.png", "0_photo.npy", "0_photo.png")
    assert sorted(p.name for p in (tmp_path / "photo").iterdir()) == sorted(
        [p.name for p in (tmp_path / "plain").iterdir()] + list(new))
    assert np.array_equal(np.load(tmp_path / "plain" / "0.npy"), np.load(tmp_path / "photo" / "0.npy"))
    err = np.load(tmp_path / "photo" / "0_photo.npy")
    assert err.shape == (96, 192) and err.dtype == np.float32
    assert bool(((err == -1) | (err >= 0)).all()) and 0 < int((err >= 0).sum()) < err.size
    assert np.asarray(Image.open(tmp_path / "photo" / "0_warped.png")).shape == (96, 192, 3)
    assert np.asarray(Image.open(tmp_path / "photo" / "0_photo.png")).shape == (96, 192)
    # with --lr_check the flagged pixels take no part
    assert P.main(base + [f"--save_path={tmp_path}/both/", "--photo_check", "--lr_check=1"]) == 0
    occ = np.asarray(Image.open(tmp_path / "both" / "0_occ.png"))
    both = np.load(tmp_path / "both" / "0_photo.npy")
    assert bool((both[occ != 0] == -1).all()) and int((both >= 0).sum()) < int((err >= 0).sum())
    assert bool((err[both >= 0] >= 0).all()), "excluding pixels brings none in"
