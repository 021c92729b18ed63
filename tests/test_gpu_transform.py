"""The training batch transform on the device (lea_train_transform_u8,
leastereo_amd/data.py) against the reference's own outputs (tests/golden/train_transform.npz,
tools/gen_golden_transform.py) and the numpy judge (tests/transform_judge.py, itself held to
that fixture bit for bit by tests/test_transform_cpu.py).

Bars.  The target is a copy and one float32 subtraction, n_valid an integer count: both equal
the judge bitwise.  The image planes are tests/test_gpu_evalio.py's arithmetic and take its
bar: the NaN pattern equal, at most 1 ulp from the numpy float64 expression, more than
99.99 % of the values equal (the device's statistics are exact integers, numpy's pairwise
float64 variance can differ in its last bits)."""
import functools
import random

import numpy as np
import pytest
import torch

from leastereo_amd import data, kernels, losses
from tests import transform_judge as J
from tests.golden_util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAXDISP = 48.0
BIG = 2 ** 31 - 1


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.array(a)).to(DEV) for a in arrays]


def run(lu, ru, dl, dr, params, ch, cw, md=MAXDISP):
    """Batched numpy inputs -> numpy (left, right, target, n_valid)."""
    lt, rt, dlt, drt = _dev(lu, ru, dl, dr)
    pt = torch.tensor(np.asarray(params).tolist(), dtype=torch.int32, device=DEV)
    out = kernels.train_transform_u8(lt, rt, dlt, drt, pt, ch, cw, md)
    assert out[0].shape == out[1].shape == (len(lu), 3, ch, cw) and out[2].shape == (len(lu), 1, ch, cw)
    assert out[3].shape == (len(lu),) and out[3].dtype == torch.int32
    return [o.cpu().numpy() for o in out]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def check_images(got, want):
    """tests/test_gpu_evalio.py's bar for (x - mean) / std."""
    assert got.shape == want.shape and got.dtype == np.float32
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    if fin.any():
        ulp = np.abs(got[fin].view(np.int32).astype(np.int64) - want[fin].view(np.int32).astype(np.int64))
        print(f"images: max ulp {ulp.max()}, equal {np.mean(got[fin] == want[fin]):.6f} of {fin.sum()}")
        assert ulp.max() <= 1
        assert np.mean(got[fin] == want[fin]) > 0.9999


def check_against(got, want_l, want_r, want_t, md=MAXDISP):
    gl, gr, gt, gn = got
    for b in range(len(gl)):
        assert same_bits(gt[b], want_t[b]), f"target of sample {b}"
        assert int(gn[b]) == J.n_valid(want_t[b], md), f"n_valid of sample {b}"
    check_images(gl, np.stack(want_l))
    check_images(gr, np.stack(want_r))


# ------------------------------------------------------------------ the reference's own crops

def fixture_case(i):
    g = golden("train_transform")
    h, w, ch, cw, ul, lr, shift, seed = (int(v) for v in g["cases"][i])
    random.seed(seed)
    params = data.sample_train_params(h, w, ch, cw, bool(ul), bool(lr), shift)
    return g, (ch, cw, bool(ul), bool(lr), shift, seed), params


@pytest.mark.parametrize("i", range(12))
def test_fixture_cases(i):
    """10x14, 5x7, 10x7, 6x8 and 6x14 images into a 6x8 crop under the (use_left, left_right,
    shift) settings the fixture lists: the device's crops are the reference's."""
    g, (ch, cw, *_), params = fixture_case(i)
    got = run(g[f"{i}/left_u8"][None], g[f"{i}/right_u8"][None], g[f"{i}/disp_left"][None],
              g[f"{i}/disp_right"][None], [params], ch, cw)
    check_against(got, [g[f"{i}/out_left"]], [g[f"{i}/out_right"]], [g[f"{i}/out_target"]])


@pytest.mark.parametrize("i,host", [(2, True), (3, False), (6, True), (8, False)])
def test_device_train_transform_returns_the_fixture_crops(i, host):
    """The public class under a seeded rng, from host arrays and from device tensors; a batch of
    two draws twice, in batch order."""
    g, (ch, cw, ul, lr, shift, seed), params = fixture_case(i)
    ins = [g[f"{i}/{k}"][None] for k in ("left_u8", "right_u8", "disp_left", "disp_right")]
    tf = data.DeviceTrainTransform(ch, cw, MAXDISP, ul, lr, shift, rng=random.Random(seed), device=DEV)
    batch = tf(*(ins if host else _dev(*ins)))
    assert isinstance(batch, data.TrainBatch) and batch.params.is_cuda and batch.params.dtype == torch.int32
    assert batch.params.cpu().tolist() == [list(params)]
    check_against([t.cpu().numpy() for t in batch[:4]], [g[f"{i}/out_left"]], [g[f"{i}/out_right"]],
                  [g[f"{i}/out_target"]])
    # the module-level generator is the default, as in the reference; two samples, two rows
    random.seed(seed)
    two = data.DeviceTrainTransform(ch, cw, MAXDISP, ul, lr, shift, device=DEV)(*(np.concatenate([a, a]) for a in ins))
    rec = random.Random(seed)
    h, w = ins[0].shape[1:3]
    rows = [list(data.sample_train_params(h, w, ch, cw, ul, lr, shift, rng=rec)) for _ in range(2)]
    assert two.params.cpu().tolist() == rows and rows[0] == list(params)
    assert same_bits(two.target[0].cpu().numpy(), g[f"{i}/out_target"])
    # training=False: no draws, test_transform's window (10x7 neither fits 6x8 nor covers it)
    if h > ch and w < cw:
        with pytest.raises(ValueError, match="test_transform"):
            data.DeviceTrainTransform(ch, cw, MAXDISP, device=DEV)(*ins, training=False)
        return
    random.seed(seed)
    state = random.getstate()
    val = data.DeviceTrainTransform(ch, cw, MAXDISP, ul, lr, shift, device=DEV)(*ins, training=False)
    assert random.getstate() == state
    assert val.params.cpu().tolist() == [list(data.center_params(h, w, ch, cw))]


# ------------------------------------------------------------------ judged shapes

# per sample: a negative shift_x (the shift path: left and right windows differ), a swap, and a
# window that hangs over the top-left pad while the target is shifted
JUDGED_PARAMS = [(5, 7, 10, -3, 0), (13, 19, 19, 0, 1), (-7, -5, -2, 3, 0)]


@functools.lru_cache(None)
def judged_inputs(ps):
    """B = 3 samples of 61x83 (an image is 15189 or 20252 bytes: sample 1 does not start on a
    16-byte boundary) and their planes, computed once."""
    rng = np.random.default_rng(61 * 83 + ps)
    lu = rng.integers(0, 256, (3, 61, 83, ps), dtype=np.uint8)
    ru = rng.integers(0, 256, (3, 61, 83, ps), dtype=np.uint8)
    dl = rng.uniform(-3, 56, (3, 61, 83)).astype(np.float32)
    dr = rng.uniform(-3, 56, (3, 61, 83)).astype(np.float32)
    planes = [J.standardize(lu[b], ru[b], dl[b], dr[b]) for b in range(3)]
    for a in (lu, ru, dl, dr, *planes):
        a.setflags(write=False)
    return lu, ru, dl, dr, planes


@pytest.mark.parametrize("ps", [3, 4])
@pytest.mark.parametrize("ch,cw", [(48, 64), (48, 62)], ids=["48x64-float4", "48x62-scalar-tail"])
def test_judged_cases(ch, cw, ps):
    """Two workgroups per image; float4 stores and the scalar tail; RGB and RGBA; each sample
    its own params row."""
    lu, ru, dl, dr, planes = judged_inputs(ps)
    got = run(lu, ru, dl, dr, JUDGED_PARAMS, ch, cw)
    want = [J.apply_params(planes[b], JUDGED_PARAMS[b], ch, cw) for b in range(3)]
    check_against(got, *zip(*want))
    assert 0 < int(got[3][0]) < ch * cw  # the mask cuts both ways at this maxdisp


def test_two_calls_give_the_same_bits():
    lu, ru, dl, dr, _ = judged_inputs(3)
    a = run(lu, ru, dl, dr, JUDGED_PARAMS, 48, 62)
    b = run(lu, ru, dl, dr, JUDGED_PARAMS, 48, 62)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_constant_channel_gives_nan_and_the_pad_stays_zero():
    """std = 0: 0 / 0 = NaN over the whole channel, as numpy; the pad around it is 0, not NaN.
    The image fits the crop, so the pad is in view; sample 1 is swapped, so the constant channel
    shows in the right input there."""
    rng = np.random.default_rng(17)
    lu = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    ru = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    lu[:, :, :, 1] = 17
    dl = rng.uniform(1, 40, (2, 9, 13)).astype(np.float32)
    rows = [(-3, -3, -3, 0, 0), (-3, -3, -3, 0, 1)]
    got = run(lu, ru, dl, None, rows, 12, 16)
    with np.errstate(all="ignore"):
        want = [J.apply_params(J.standardize(lu[b], ru[b], dl[b]), rows[b], 12, 16, has_right_disp=False)
                for b in range(2)]
    check_against(got, *zip(*want))
    assert np.isnan(got[0][0, 1, 3:, 3:]).all() and np.isnan(got[1][1, 1, 3:, 3:]).all()
    for planes in (got[0][0], got[1][1]):
        assert (planes[:, :3, :] == 0).all() and (planes[:, :, :3] == 0).all()
    # a swap without a right disparity: the target is all pad (0), nothing valid
    assert (got[2][1] == 0).all() and int(got[3][1]) == 0
    assert int(got[3][0]) == 9 * 13


# ------------------------------------------------------------------ the validation side

@pytest.mark.parametrize("h,w", [(30, 40), (50, 60)], ids=["pad", "crop"])
def test_center_params_equals_standardize_crop_u8(h, w):
    """test_transform's window through the training entry: the images equal the inference
    entry's bit for bit (same table, same window), the target the judge's test_transform."""
    ch, cw = 32, 48
    rng = np.random.default_rng(h)
    lu = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    ru = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    dl = rng.uniform(-3, 56, (2, h, w)).astype(np.float32)
    rows = [data.center_params(h, w, ch, cw)] * 2
    got = run(lu, ru, dl, None, rows, ch, cw)
    ref_l, ref_r = kernels.standardize_crop_u8(*_dev(lu, ru), ch, cw)
    assert np.array_equal(got[0].view(np.int32), ref_l.cpu().numpy().view(np.int32))
    assert np.array_equal(got[1].view(np.int32), ref_r.cpu().numpy().view(np.int32))
    for b in range(2):
        want_t = J.test_transform(J.standardize(lu[b], ru[b], dl[b]), ch, cw)[2]
        assert same_bits(got[2][b], np.ascontiguousarray(want_t))
        assert int(got[3][b]) == J.n_valid(want_t, MAXDISP)


# ------------------------------------------------------------------ params the entry cannot check

def test_hostile_params_give_pad():
    """Defined behaviour for any five ints: the source coordinates are formed in 64 bits and
    tested against the image before every read, so windows far outside it are all pad; unknown
    flag bits are ignored.  maxdisp 2000 makes the 1000 pad count as valid."""
    lu, ru, dl, dr, planes = judged_inputs(3)
    rows = [(BIG, 0, 0, 0, 0), (0, -BIG, BIG, BIG, 0x7FFFFFFE), (-BIG, BIG, -BIG, -BIG, 1 | 0x70)]
    got = run(lu, ru, dl, dr, rows, 48, 62, md=2000.0)
    want = [J.apply_params(planes[b], rows[b], 48, 62) for b in range(3)]
    for b in range(3):
        assert not want[b][0].any() and not want[b][1].any()  # the judge agrees: nothing in view
    check_against(got, *zip(*want), md=2000.0)
    assert not got[0].any() and not got[1].any()
    assert (got[2][0] == 1000).all() and got[3].tolist() == [48 * 62, 0, 0]
    # unknown bits alone change nothing
    a = run(lu, ru, dl, dr, JUDGED_PARAMS, 48, 62)
    b = run(lu, ru, dl, dr, [r[:4] + (r[4] | 0x7FFFFFF0,) for r in JUDGED_PARAMS], 48, 62)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_graph_capture_replays_with_fresh_params():
    """One stream, no parallel branches.  The params are read from device memory, so a replay
    after overwriting the static buffer cuts the new crops; a capture cannot contain a host
    synchronisation, so this also shows the entry has none."""
    lu, ru, dl, dr, _ = judged_inputs(4)
    second = [(0, 0, 3, -3, 0), (-20, 30, 30, 0, 1), (13, 19, 19, 0, 0)]
    eager = [run(lu, ru, dl, dr, rows, 48, 64) for rows in (JUDGED_PARAMS, second)]
    lt, rt, dlt, drt = _dev(lu, ru, dl, dr)
    static = torch.zeros(3, 5, dtype=torch.int32, device=DEV)

    def step():
        return kernels.train_transform_u8(lt, rt, dlt, drt, static, 48, 64, MAXDISP)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for rows, want in ((JUDGED_PARAMS, eager[0]), (second, eager[1]), (JUDGED_PARAMS, eager[0])):
        static.copy_(torch.tensor(rows, dtype=torch.int32))
        graph.replay()
        for got, w in zip(out, want):
            assert np.array_equal(got.cpu().numpy().view(np.uint8), w.view(np.uint8))
    assert not np.array_equal(eager[0][2], eager[1][2])


# ------------------------------------------------------------------ into a train step

def test_whole_model_train_step_on_the_transform_output():
    """train.py:150-158 fed by the device transform at tests/test_gpu_training.py's whole-model
    shape (96x192, maxdisp 48): model.train(), model(left, right), the masked smooth-L1,
    backward -- a finite loss and finite, non-zero gradients."""
    from leastereo_amd.config import LEAStereoArgs, default_arch_args
    from leastereo_amd.model import LEAStereo
    from tests.golden_util import state_dict
    rng = np.random.default_rng(96)
    lu = rng.integers(0, 256, (1, 100, 200, 3), dtype=np.uint8)
    ru = rng.integers(0, 256, (1, 100, 200, 3), dtype=np.uint8)
    dl = rng.uniform(1, 60, (1, 100, 200)).astype(np.float32)
    tf = data.DeviceTrainTransform(96, 192, 48, shift=3, rng=random.Random(5), device=DEV)
    batch = tf(lu, ru, dl)
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=48)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    m = m.to(DEV).train()
    left = batch.left.requires_grad_(True)
    disp = m(left, batch.right)
    loss = losses.masked_smooth_l1(disp, batch.target, 48)
    loss.backward()
    n = int(batch.n_valid[0])
    mask = (batch.target < 48) & (batch.target > 0.001)
    assert n == int(mask.sum()) and 0 < n < 96 * 192
    assert torch.isfinite(loss.detach()).item() and float(loss.detach()) > 0
    assert torch.isfinite(left.grad).all() and float(left.grad.abs().max()) > 0
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
