"""The edge-aware training loss on the GPU: lea_median5x5_f32, lea_edge_loss_f32 and
lea_edge_loss_grad_f32 through kernels.median_blur5 / edge_loss_sums / edge_loss_grad and
leastereo_amd.losses.

The median is compared bit for bit, every pixel, with the sort-based numpy judge
(tests/loss_judge.py).  The loss and its gradient are compared with the reference's own
expressions in float64 torch on the CPU; the bar is the project's convention
(test_gpu_lr.py, test_gpu_disp_stats.py): an error against fp64 of at most
max(4 x E_cpu32, 8 ulp_f32 of the quantity), E_cpu32 being the same judge run in float32 on
the CPU for that very case.  8 ulp: a term of the entry is a handful of f32 operations
(a subtraction, a product or two, expf), each within an ulp of the term, and a mean of such
terms, taken in float64, cannot be further off than its worst term.

Shapes are the smallest that reach each path.  The median's tile is 32 wide and 16 tall
(kMedTW, kMedTH in csrc/median.hip), so (1, 17, 33) is one row and one column more; the
loss kernels' tile is 64 x 16 (kElW, kElH in csrc/edge_loss.hip), so (1, 17, 65) is.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from leastereo_amd import _lib, kernels, losses
from tests import loss_judge

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEDIAN_SHAPES = [(1, 1, 1),     # smallest legal image
                 (2, 3, 7),     # smaller than the window, batch stride
                 (1, 2, 9),     # smaller than the window in H only
                 (1, 6, 5),     # W equal to the window
                 (2, 17, 70),   # crosses a tile in W, odd sizes, batch stride larger than H*W
                 (1, 17, 33)]   # the 32 x 16 tile plus one row and one column
LOSS_SHAPES = [(1, 3, 3),       # a single edge position
               (2, 5, 8),
               (2, 17, 70),
               (1, 17, 65)]     # the 64 x 16 tile plus one row and one column
IDS = dict(ids=lambda s: "x".join(map(str, s)))


def blocks(rng, shape, bh, bw, levels, step):
    """Piecewise constant: bh x bw blocks of ``levels`` values, multiples of ``step``."""
    b, h, w = shape
    coarse = rng.integers(0, levels, (b, -(-h // bh), -(-w // bw)))
    return (np.kron(coarse, np.ones((1, bh, bw)))[:, :h, :w] * step).astype(np.float32)


@functools.lru_cache(None)
def median_input(shape, kind):
    rng = np.random.default_rng(5)
    if kind == "normal":
        return (20.0 * rng.standard_normal(shape)).astype(np.float32)
    x = blocks(rng, shape, 3, 4, 4, 7.5)        # ties everywhere
    x[:, : max(1, shape[1] // 2), : max(1, shape[2] // 3)] = 0.0
    return x


@functools.lru_cache(None)
def median_judge(shape, kind, iterations):
    return loss_judge.median_blur(median_input(shape, kind), iterations)


def to_device(x, padded_batch_stride=False):
    t = torch.from_numpy(x)
    if not padded_batch_stride:
        return t.to(DEV)
    b, h, w = t.shape
    buf = torch.full((b, h * w + 11), -777.0, device=DEV)
    buf[:, : h * w] = t.reshape(b, -1).to(DEV)
    v = buf[:, : h * w].view(b, h, w)
    assert v.stride() == (h * w + 11, w, 1)
    return v


@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("kind", ["normal", "blocks"])
@pytest.mark.parametrize("shape", MEDIAN_SHAPES, **IDS)
def test_median_bit_for_bit(shape, kind, iterations):
    x = median_input(shape, kind)
    want = median_judge(shape, kind, iterations)
    got = kernels.median_blur5(to_device(x, padded_batch_stride=shape == (2, 17, 70)), iterations)
    assert got.shape == shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{shape} {kind} iterations {iterations}: {bad} of {got.size} pixels differ")
    assert bad == 0
    if iterations == 2 and shape == (2, 17, 70) and kind == "normal":
        wrong = loss_judge.median_twice_of_wide_replicate(x)
        n = int((wrong != want).sum())
        print(f"the valid median of the 4-wide replicated input differs in {n} pixels")
        assert n > 0 and int((got != wrong).sum()) == n


def test_median_2d_and_smooth_target():
    x = median_input((2, 17, 70), "normal")
    dev = to_device(x)
    got = kernels.median_blur5(dev[1], 2)
    assert got.shape == (17, 70)
    assert np.array_equal(got.cpu().numpy(), median_judge((2, 17, 70), "normal", 2)[1])
    assert torch.equal(losses.smooth_target(dev), kernels.median_blur5(dev, 2))
    assert losses.make_smoother_disp is losses.smooth_target
    with pytest.raises(ValueError):
        kernels.median_blur5(dev, 3)
    y = torch.empty_like(dev)
    lib = _lib.load()
    assert lib.lea_median5x5_f32(dev.data_ptr(), 17 * 70, dev.data_ptr() + 4, 17 * 70, 2, 17, 70, 2, None) == 1001
    assert lib.lea_median5x5_f32(dev.data_ptr(), 17 * 70 - 1, y.data_ptr(), 17 * 70, 2, 17, 70, 2, None) == 1001


# ------------------------------------------------------------------ loss and gradient

W_EDGE = 0.2


def maxdisp_of(shape):
    return 48.0


@functools.lru_cache(None)
def loss_case(shape, kind):
    """Inputs and both judges of one case, computed once and left unchanged."""
    rng = np.random.default_rng(11)
    b, h, w = shape
    target = rng.uniform(0.0, 60.0, shape).astype(np.float32)      # some >= maxdisp 48
    target[:, : max(1, h // 3), : max(1, w // 3)] = 0.0            # occlusions
    if kind == "invalid":
        target = np.where(rng.random(shape) < 0.5, 0.0, 100.0).astype(np.float32)
    if kind == "blocks":
        # multiples of 0.5 below 64: every partial sum of a Sobel response is exact in f32
        # too, so the float32 judge sees the same signs as the float64 one
        pred = blocks(rng, shape, 6, 10, 100, 0.5)
    else:
        pred = (target + 1.5 * rng.standard_normal(shape)).astype(np.float32)
    ts = loss_judge.median_blur(target, 2)
    md = maxdisp_of(shape)
    pred, target, ts = torch.from_numpy(pred), torch.from_numpy(target), torch.from_numpy(ts)
    j64 = loss_judge.torch_loss(pred, target, ts, md, W_EDGE, torch.float64)
    j32 = loss_judge.torch_loss(pred, target, ts, md, W_EDGE, torch.float32)
    return dict(pred=pred.to(DEV), target=target.to(DEV), ts=ts.to(DEV), md=md, j64=j64, j32=j32,
                n=int(((target < md) & (target > 0.001)).sum()))


def ulp_of(x):
    return float(np.spacing(np.float32(abs(x))))


def run_entries(c, scales=(1.0, W_EDGE)):
    sums = kernels.edge_loss_sums(c["pred"], c["target"], c["ts"], c["md"])
    grad = kernels.edge_loss_grad(c["pred"], c["target"], c["ts"], c["md"], sums,
                                  torch.tensor(scales, device=DEV, dtype=torch.float32))
    return sums, grad


CASES = [(s, "noise") for s in LOSS_SHAPES] + [((2, 17, 70), "blocks")]


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_loss_and_gradient_against_fp64(shape, kind):
    c = loss_case(shape, kind)
    b, h, w = shape
    sums, grad = run_entries(c)
    assert sums.dtype == torch.float64 and sums.is_cuda and grad.shape == shape and grad.dtype == torch.float32
    s = sums.cpu().tolist()
    assert s[0] == c["n"] and 0 < c["n"] < b * h * w, "both mask edges bite"
    d = c["pred"] - c["target"]
    m = (c["target"] < c["md"]) & (c["target"] > 0.001)
    if b * h * w >= 80:  # a 3 x 3 map has too few pixels to promise either
        assert bool((d[m].abs() < 1).any()) and bool((d[m].abs() > 1).any()), "both smooth-L1 branches occur"
        assert bool((c["target"] >= c["md"]).any()) and bool((c["target"] <= 0.001).any())
    direct, edge = s[1] / s[0], s[3] / (b * (h - 2) * (w - 2))
    comb = direct + W_EDGE * edge
    d64, e64, c64, g64 = c["j64"]
    d32, e32, c32, g32 = c["j32"]
    # the train loop's EPE: one f32 subtraction per term, each within 2^-24 of its value
    assert s[2] / s[0] == pytest.approx(float(d[m].double().abs().mean()), rel=1e-6)
    rows = [("direct", direct, d64, d32), ("edge", edge, e64, e32), ("combined", comb, c64, c32)]
    fails = []
    for name, got, want, cpu32 in rows:
        e_gpu, e_cpu = abs(got - want), abs(cpu32 - want)
        bar = max(4 * e_cpu, 8 * ulp_of(want))
        print(f"{shape} {kind} {name}: fp64 {want:.9g} gpu err {e_gpu:.3e} cpu32 err {e_cpu:.3e} bar {bar:.3e}")
        if not e_gpu <= bar:
            fails.append((name, e_gpu, bar))
    gmax = float(g64.abs().max())
    e_gpu = float((grad.cpu().double() - g64).abs().max())      # every pixel
    e_cpu = float((g32.double() - g64).abs().max())
    bar = max(4 * e_cpu, 8 * ulp_of(gmax))
    print(f"{shape} {kind} gradient: max |g| {gmax:.6g} gpu err {e_gpu:.3e} cpu32 err {e_cpu:.3e} bar {bar:.3e}")
    assert torch.isfinite(grad).all()
    if not e_gpu <= bar:
        fails.append(("gradient", e_gpu, bar))
    assert not fails, fails


def test_edge_gradient_is_exactly_zero_inside_constant_regions():
    from scipy import ndimage
    c = loss_case((2, 17, 70), "blocks")
    _, g_edge = run_entries(c, scales=(0.0, 1.0))
    p = c["pred"].cpu().numpy()
    flat = np.stack([ndimage.maximum_filter(i, size=5, mode="nearest") == ndimage.minimum_filter(i, size=5, mode="nearest")
                     for i in p])
    assert 50 < int(flat.sum()) < flat.size
    g = g_edge.cpu().numpy()
    assert bool((g[flat] == 0).all())
    assert bool((g[~flat] != 0).any())


def test_all_invalid_target():
    shape = (2, 17, 70)
    c = loss_case(shape, "invalid")
    assert c["n"] == 0
    sums, grad = run_entries(c)
    s = sums.cpu().tolist()
    assert s[0] == 0 and s[1] == 0 and s[2] == 0
    _, g_edge_only = run_entries(c, scales=(0.0, W_EDGE))
    assert torch.equal(grad, g_edge_only), "the direct term's gradient is exactly 0"
    assert torch.isfinite(grad).all()
    d64, e64, c64, g64 = c["j64"]
    d32, e32, c32, g32 = c["j32"]
    assert d64 is None
    edge = s[3] / (2 * 15 * 68)
    e_gpu, e_cpu = abs(edge - e64), abs(e32 - e64)
    print(f"all invalid: edge fp64 {e64:.9g} gpu err {e_gpu:.3e} cpu32 err {e_cpu:.3e}")
    assert e_gpu <= max(4 * e_cpu, 8 * ulp_of(e64))
    g_gpu, g_cpu = float((grad.cpu().double() - g64).abs().max()), float((g32.double() - g64).abs().max())
    print(f"all invalid: gradient gpu err {g_gpu:.3e} cpu32 err {g_cpu:.3e}")
    assert g_gpu <= max(4 * g_cpu, 8 * ulp_of(float(g64.abs().max())))
    # the wrapper: a finite loss and gradient where torch's empty mean is NaN
    pred = c["pred"].clone().requires_grad_()
    loss, (direct, _, epe, n) = losses.combined_loss(pred, c["target"], c["md"], W_EDGE, return_parts=True)
    loss.backward()
    assert float(direct.detach()) == 0 and float(epe) == 0 and float(n) == 0 and torch.equal(pred.grad, grad)


# ------------------------------------------------------------------ determinism, capture

def test_two_runs_give_identical_bits():
    c = loss_case((2, 17, 70), "noise")
    a = (kernels.median_blur5(c["target"], 2),) + run_entries(c)
    b = (kernels.median_blur5(c["target"], 2),) + run_entries(c)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_graph_capture_replays_the_eager_calls():
    """A capture cannot contain a host synchronisation or a read-back: this is also the
    test that none of the three entries does either."""
    shape = (2, 17, 70)
    first, second = loss_case(shape, "blocks"), loss_case(shape, "noise")
    pred, target = first["pred"].clone(), first["target"].clone()
    scales = torch.tensor([1.0, W_EDGE], device=DEV)
    md = first["md"]

    def step():
        ts = kernels.median_blur5(target, 2)
        sums = kernels.edge_loss_sums(pred, target, ts, md)
        return ts, sums, kernels.edge_loss_grad(pred, target, ts, md, sums, scales)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for c in (second, first):
        pred.copy_(c["pred"])
        target.copy_(c["target"])
        graph.replay()
        want = (kernels.median_blur5(c["target"], 2),) + run_entries(c)
        assert torch.equal(want[0], c["ts"])
        for got, w in zip(out, want):
            assert torch.equal(got.view(torch.uint8), w.view(torch.uint8))


# ------------------------------------------------------------------ the autograd wrapper

def test_combined_loss_backward_is_the_grad_entry():
    c = loss_case((2, 17, 70), "noise")
    sums, want = run_entries(c)
    pred = c["pred"].clone().requires_grad_()
    target = c["target"].clone().requires_grad_()
    loss, (direct, grad, epe, n) = losses.combined_loss(pred, target, c["md"], W_EDGE, return_parts=True)
    for t in (loss, direct, grad, epe, n):
        assert t.is_cuda and t.dim() == 0
    loss.backward()
    assert torch.equal(pred.grad, want) and target.grad is None
    s = sums.cpu().tolist()
    assert float(n) == s[0]
    assert float(direct) == pytest.approx(s[1] / s[0], rel=1e-6) and float(epe) == pytest.approx(s[2] / s[0], rel=1e-6)
    assert float(grad) == pytest.approx(s[3] / (2 * 15 * 68), rel=1e-6)
    assert float(loss) == pytest.approx(c["j64"][2], rel=1e-5)
    # the plain call returns the loss alone; [B, 1, H, W] maps are taken as the reference's squeeze does
    assert torch.equal(losses.combined_loss(c["pred"].unsqueeze(1), c["target"], c["md"], W_EDGE), loss.detach())


def test_zero_edge_weight_is_masked_smooth_l1():
    c = loss_case((2, 17, 70), "noise")
    p0, p1 = c["pred"].clone().requires_grad_(), c["pred"].clone().requires_grad_()
    a = losses.combined_loss(p0, c["target"], c["md"], grad_loss_w=0)
    b = losses.masked_smooth_l1(p1, c["target"], c["md"])
    a.backward()
    b.backward()
    assert torch.equal(a, b) and torch.equal(p0.grad, p1.grad)
    m = (c["target"] < c["md"]) & (c["target"] > 0.001)
    assert float(b) == pytest.approx(float(F.smooth_l1_loss(c["pred"][m], c["target"][m])), rel=1e-5)


def test_gradient_aware_loss2_is_the_edge_term():
    c = loss_case((2, 17, 70), "noise")
    p = c["pred"].clone().requires_grad_()
    e = losses.gradient_aware_loss2(p, c["target"], device="ignored")
    e.backward()
    assert float(e) == pytest.approx(c["j64"][1], rel=1e-5)
    _, want = run_entries(c, scales=(0.0, 1.0))
    assert torch.equal(p.grad, want)
