"""Whole-scene inference on the GPU: the tile gather (lea_standardize_tiles_u8) bit for bit
against slices of the standardised scene, the blend (lea_tile_blend_f32) bit for bit against
the numpy judge (tests/scene_judge.py), scene.SceneRunner / LEAStereo.forward_scene against
the judge's blend of the model's own per-batch outputs, and predict --scene.

The small case throughout: maxdisp 48, tile 96 x 192, context 8, ramp 8.  One bound is not
an equality: with every tile cut from one scene-wide map M the blend must give M back to
within (n + 2) * 2^-24 * |M| at a pixel of n covering tiles (n products, n - 1 adds and one
divide, each rounded once, the integer weights and their sums exact), and exactly where n = 1.
"""
import functools

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels, scene
from leastereo_amd.config import LEAStereoArgs, default_arch_args
from leastereo_amd.model import LEAStereo
from tests import scene_judge as J
from tests.golden_util import golden, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
TH, TW, MD, CTX, RAMP = 96, 192, 48, 8, 8
KW = dict(context=CTX, ramp=RAMP)


def _scene_u8(h, w, c, seed):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.integers(0, 256, (h, w, c), dtype=np.uint8)).to(DEV),
            torch.from_numpy(rng.integers(0, 256, (h, w, c), dtype=np.uint8)).to(DEV))


def _cut(full, oy, ox):
    """The TH x TW window of full [3, H, W] at (oy, ox), 0 outside it (host)."""
    _, h, w = full.shape
    out = torch.zeros((3, TH, TW), dtype=full.dtype)
    y0, y1, x0, x1 = max(oy, 0), min(oy + TH, h), max(ox, 0), min(ox + TW, w)
    if y0 < y1 and x0 < x1:
        out[:, y0 - oy:y1 - oy, x0 - ox:x1 - ox] = full[:, y0:y1, x0:x1]
    return out


# ------------------------------------------------------------------ gather
@pytest.mark.parametrize("shape", [(150, 300, 3), (80, 300, 4)], ids=lambda s: "x".join(map(str, s)))
def test_gather_equals_slices_of_the_standardised_scene(shape):
    h, w, c = shape
    left, right = _scene_u8(h, w, c, 5)
    plan = scene.plan_tiles(h, w, TH, TW, MD, **KW)
    # every tile of the plan, then origins that straddle each border and lie wholly outside
    extra = [(-5, -7), (h - 10, w - 20), (h, 0), (0, w), (-TH, 0), (0, -TW), (10 ** 6, 3), (3, -10 ** 6),
             (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)]
    origins = plan.origins.tolist() + [list(o) for o in extra]
    got_l, got_r = kernels.standardize_tiles_u8(left, right, torch.tensor(origins, dtype=torch.int32, device=DEV),
                                                TH, TW)
    assert got_l.shape == got_r.shape == (len(origins), 3, TH, TW) and got_l.dtype == torch.float32
    # the full-size crop of standardize_crop_u8 is the whole standardised scene
    full_l, full_r = (t[0].cpu() for t in kernels.standardize_crop_u8(left, right, h, w))
    for k, (oy, ox) in enumerate(origins):
        assert torch.equal(got_l[k].cpu(), _cut(full_l, oy, ox)), (k, oy, ox)
        assert torch.equal(got_r[k].cpu(), _cut(full_r, oy, ox)), (k, oy, ox)
    for k in range(len(plan) + 4, len(origins)):  # wholly outside: all zero
        assert not got_l[k].any() and not got_r[k].any(), origins[k]
    # the scene's statistics, not the tile's: a tile is not standardised on its own
    if h >= TH:
        own = kernels.standardize_crop_u8(left[:TH, :TW].contiguous(), right[:TH, :TW].contiguous(), TH, TW)[0]
        assert not torch.equal(own[0], got_l[0])


def test_gather_at_the_centre_crop_origin_is_standardize_crop():
    h, w = 150, 300
    left, right = _scene_u8(h, w, 3, 6)
    o = torch.tensor([[(h - TH) // 2, (w - TW) // 2]], dtype=torch.int32, device=DEV)
    got = kernels.standardize_tiles_u8(left, right, o, TH, TW)
    want = kernels.standardize_crop_u8(left, right, TH, TW)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a tile width that is no multiple of 4 takes the scalar stores
    got = kernels.standardize_tiles_u8(left, right, o, TH - 1, TW - 3)
    assert torch.equal(got[0], want[0][:, :, :TH - 1, :TW - 3]) and torch.equal(got[1], want[1][:, :, :TH - 1, :TW - 3])


def test_gather_refusals():
    left, right = _scene_u8(20, 30, 3, 7)
    o = torch.zeros((1, 2), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.HipKernelError):
        kernels.standardize_tiles_u8(left.cpu(), right, o, TH, TW)
    with pytest.raises(_lib.HipKernelError):
        kernels.standardize_tiles_u8(left, right, o.long(), TH, TW)
    with pytest.raises(ValueError):
        kernels.standardize_tiles_u8(left, right[:10], o, TH, TW)
    with pytest.raises(ValueError):
        kernels.standardize_tiles_u8(left, right, o[:0], TH, TW)


# ------------------------------------------------------------------ blend
BLEND_SIZES = [(150, 300), (80, 300), (96, 192), (97, 193), (300, 700)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _judge(tiles, plan, view):
    return J.blend(tiles, plan.ys, plan.xs, plan.height, plan.width, plan.maxdisp, plan.context, plan.ramp, view)


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("size", BLEND_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_blend_equals_the_judge(size, view):
    h, w = size
    plan = scene.plan_tiles(h, w, TH, TW, MD, **KW)
    rng = np.random.default_rng(h * 7 + w + (view == "right"))
    tiles = rng.standard_normal((len(plan), TH, TW)).astype(np.float32)
    for k in range(len(plan)):  # a NaN wherever the weight is 0: it must not reach the result
        tiles[k][plan.weights(k, view) == 0] = np.nan
    want, n = _judge(tiles, plan, view)
    assert n.min() >= 1 and np.isfinite(want).all()
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    got = kernels.blend_tiles(torch.from_numpy(tiles).to(DEV), plan, view, count=count).cpu().numpy()
    assert got.shape == (h, w) and got.dtype == np.float32
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    assert int(count.item()) == 0
    # the same through a batch stride that is not the tile's size, checked
    buf = torch.full((len(plan), TH * TW + 64), float("nan"), device=DEV)
    buf[:, :TH * TW] = torch.from_numpy(tiles).to(DEV).flatten(1)
    strided = buf[:, :TH * TW].unflatten(1, (TH, TW))
    assert len(plan) == 1 or strided.stride() == (TH * TW + 64, TW, 1)
    got2 = kernels.blend_tiles(strided, plan, view, check=True).cpu().numpy()
    assert np.array_equal(_bits(got2), _bits(want))


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("size", BLEND_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_blend_of_one_map_gives_it_back(size, view):
    h, w = size
    plan = scene.plan_tiles(h, w, TH, TW, MD, **KW)
    rng = np.random.default_rng(h + w)
    m = (rng.standard_normal((h, w)) * 40.0).astype(np.float32)
    tiles = np.stack([_cut(torch.from_numpy(m)[None].expand(3, -1, -1), oy, ox)[0].numpy()
                      for oy, ox in plan.origins.tolist()])
    got = kernels.blend_tiles(torch.from_numpy(tiles).to(DEV), plan, view).cpu().numpy()
    n = plan.cover_count(view)
    err = np.abs(got.astype(np.float64) - m.astype(np.float64))
    bound = (n + 2) * 2.0 ** -24 * np.abs(m.astype(np.float64))
    print(f"{h}x{w} {view}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, "
          f"{int((n > 1).sum())} blended pixels, max cover {int(n.max())}")
    assert (err <= bound).all()
    assert np.array_equal(_bits(got)[n == 1], _bits(m)[n == 1])


def test_blend_counts_a_hole():
    """Origins handed in directly: the right 116 columns of a 150 x 300 scene have no tile."""
    plan = scene.TilePlan(150, 300, TH, TW, MD, CTX, RAMP, [0, 54], [0])
    assert not plan.covers()
    tiles = np.random.default_rng(3).standard_normal((2, TH, TW)).astype(np.float32)
    want, n = _judge(tiles, plan, "left")
    assert int((n == 0).sum()) == 150 * (300 - (TW - CTX))
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev_tiles = torch.from_numpy(tiles).to(DEV)
    got = kernels.blend_tiles(dev_tiles, plan, "left", count=count).cpu().numpy()
    assert int(count.item()) == int((n == 0).sum()) > 0
    assert np.array_equal(_bits(got), _bits(want)) and not got[n == 0].any()
    # the count is cleared by every call, and asked for only where the caller asks
    kernels.blend_tiles(dev_tiles, plan, "left", count=count)
    assert int(count.item()) == int((n == 0).sum())
    kernels.blend_tiles(dev_tiles, plan, "left")
    with pytest.raises(_lib.HipKernelError, match="no covering tile"):
        kernels.blend_tiles(dev_tiles, plan, "left", check=True)
    with pytest.raises(ValueError):
        kernels.blend_tiles(dev_tiles[:1], plan, "left")
    with pytest.raises(ValueError):
        kernels.blend_tiles(dev_tiles, plan, "up")


# ------------------------------------------------------------------ model level
@functools.lru_cache(maxsize=None)
def _model():
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV).eval()


def _golden_pair(h, w):
    g = golden("c1_sceneflow")
    return (torch.from_numpy(np.ascontiguousarray(g["left_u8"][:h, :w])).to(DEV),
            torch.from_numpy(np.ascontiguousarray(g["right_u8"][:h, :w])).to(DEV))


def test_a_scene_of_one_tile_is_the_plain_forward():
    m = _model()
    left, right = _golden_pair(TH, TW)
    with torch.no_grad():
        want = m(*kernels.standardize_crop_u8(left, right, TH, TW))[0]
    res = m.forward_scene(left, right, tile=(TH, TW), **KW)
    assert isinstance(res, scene.SceneResult) and res.disp.shape == (TH, TW)
    assert torch.equal(res.disp, want)
    assert all(v is None for v in res[1:])
    # host scenes (numpy) go up as they are
    res = m.forward_scene(left.cpu().numpy(), right.cpu().numpy(), tile=(TH, TW), **KW)
    assert torch.equal(res.disp, want)


def _judge_of_batches(runner, left, right, call, names):
    """The judge's blend of ``call`` run on exactly the batches the runner forms."""
    plan = runner.plan(left.shape[0], left.shape[1])
    xl, xr = runner.tiles(left, right)
    b = runner.tile_batch
    assert xl.shape == (len(runner.batches(plan)) * b, 3, TH, TW)
    tiles = {name: np.zeros((len(plan), TH, TW), dtype=np.float32) for name in names}
    for i, idx in enumerate(runner.batches(plan)):
        with torch.no_grad():
            out = call(xl[i * b:(i + 1) * b], xr[i * b:(i + 1) * b])
        for j, k in enumerate(idx):
            if k < 0:  # a pad tile: zeros in, never blended
                assert not xl[i * b + j].any() and not xr[i * b + j].any()
                continue
            for name in names:
                tiles[name][k] = getattr(out, name)[j].cpu().numpy()
    return {name: _judge(tiles[name], plan, "right" if name == "disp_right" else "left")[0] for name in names}


@pytest.mark.parametrize("tile_batch", [1, 3])
def test_scene_equals_the_judge_blend_of_the_models_tiles(tile_batch):
    m = _model()
    left, right = _golden_pair(150, 300)
    runner = scene.SceneRunner(m, TH, TW, tile_batch=tile_batch, **KW)
    assert runner.batches(runner.plan(150, 300)) == ([[0], [1], [2], [3]] if tile_batch == 1 else
                                                     [[0, 1, 2], [3, -1, -1]])
    res = runner(left, right)
    Plain = type("Plain", (), {})

    def plain(x, y):
        o = Plain()
        o.disp = m(x, y)
        return o
    want = _judge_of_batches(runner, left, right, plain, ["disp"])
    assert res.disp.shape == (150, 300) and res.entropy is None and res.disp_right is None
    assert np.array_equal(_bits(res.disp.cpu().numpy()), _bits(want["disp"]))
    # with the confidence maps: the same disparity, and each map the judge's blend
    conf = scene.SceneRunner(m, TH, TW, tile_batch=tile_batch, confidence=True, radius=3, **KW)
    got = conf(left, right)
    names = ["disp", "entropy", "peak", "disp_local"]
    want = _judge_of_batches(conf, left, right, lambda x, y: m.forward_with_confidence(x, y, 3), names)
    for name in names:
        assert np.array_equal(_bits(getattr(got, name).cpu().numpy()), _bits(want[name])), name
    assert torch.equal(got.disp, res.disp)


def test_scene_lr_check_runs_once_on_the_blended_maps():
    m = _model()
    left, right = _golden_pair(150, 300)
    plain = scene.SceneRunner(m, TH, TW, tile_batch=3, **KW)(left, right)
    runner = scene.SceneRunner(m, TH, TW, tile_batch=3, lr_threshold=1.0, **KW)
    res = runner(left, right)
    assert torch.equal(res.disp, plain.disp)
    want = _judge_of_batches(runner, left, right, lambda x, y: m.forward_lr(x, y, 1.0), ["disp", "disp_right"])
    assert np.array_equal(_bits(res.disp_right.cpu().numpy()), _bits(want["disp_right"]))
    lr = kernels.lr_check(res.disp[None], res.disp_right[None], 1.0)
    assert torch.equal(res.state, lr.state[0]) and torch.equal(res.disp_filled, lr.disp_filled[0])
    assert res.state.dtype == torch.uint8 and set(res.state.unique().tolist()) <= {0, 1, 2}
    assert res.state.shape == res.disp_filled.shape == (150, 300)
    # together with the confidence maps: the same maps again
    both = scene.SceneRunner(m, TH, TW, tile_batch=3, lr_threshold=1.0, confidence=True, **KW)(left, right)
    assert torch.equal(both.disp, res.disp) and torch.equal(both.disp_right, res.disp_right)
    assert torch.equal(both.state, res.state) and both.entropy is not None


def test_graph_replays_what_the_direct_calls_give():
    m = _model()
    left, right = _golden_pair(150, 300)
    graphed = scene.SceneRunner(m, TH, TW, tile_batch=2, graph=True, **KW)
    direct = scene.SceneRunner(m, TH, TW, tile_batch=2, graph=False, **KW)
    a, b = graphed(left, right), direct(left, right)
    assert torch.equal(a.disp, b.disp)
    assert graphed.captures == 1 and direct.captures == 0
    # a second scene of the same size replays: no new capture, its own result
    g = golden("c1_sceneflow")
    left2 = torch.from_numpy(np.ascontiguousarray(g["left_u8"][100:250, 200:500])).to(DEV)
    right2 = torch.from_numpy(np.ascontiguousarray(g["right_u8"][100:250, 200:500])).to(DEV)
    a2 = graphed(left2, right2)
    assert graphed.captures == 1
    assert torch.equal(a2.disp, direct(left2, right2).disp) and not torch.equal(a2.disp, a.disp)
    # another size makes another plan, the same graph
    a3 = graphed(left2[:120, :250].contiguous(), right2[:120, :250].contiguous())
    assert graphed.captures == 1 and a3.disp.shape == (120, 250)


def test_scene_is_inference_only():
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV).to(DEV)
    left, right = _golden_pair(TH, TW)
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_scene(left, right, tile=(TH, TW), graph=False, **KW)
    m.eval()
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_scene(left.float().requires_grad_(), right.float(), tile=(TH, TW), graph=False, **KW)
    with pytest.raises(ValueError, match="uint8"):
        m.forward_scene(left.float(), right.float(), tile=(TH, TW), graph=False, **KW)
    with pytest.raises(ValueError):  # a tile the network cannot run
        scene.SceneRunner(m, 40, 64)


# ------------------------------------------------------------------ CLI
def test_predict_cli_scene(tmp_path):
    """A 150 x 300 sceneflow-layout pair: --scene 1 writes maps of the scene's size, equal to
    forward_scene; without it the output is the 96 x 192 centre crop it is today."""
    from PIL import Image
    from leastereo_amd import predict as P
    g = golden("c1_sceneflow")
    for side in ("left", "right"):
        d = tmp_path / "frames_finalpass" / "S" / side
        d.mkdir(parents=True)
        Image.fromarray(g[side + "_u8"][:150, :300]).save(d / "0001.png")
    (tmp_path / "list.txt").write_text("S/left/0001.png\n")
    torch.save({"state_dict": {"module." + k: v for k, v in state_dict().items()}}, tmp_path / "ckpt.pth")
    base = ["--sceneflow=1", f"--maxdisp={MD}", "--crop_height=96", "--crop_width=192",
            f"--data_path={tmp_path}/", f"--test_list={tmp_path}/list.txt", f"--resume={tmp_path}/ckpt.pth"]
    flags = ["--scene", "1", "--scene_context=8", "--scene_ramp=8", "--scene_batch=2"]
    assert P.main(base + [f"--save_path={tmp_path}/plain/"]) == 0
    assert P.main(base + flags + [f"--save_path={tmp_path}/scene/"]) == 0
    assert np.load(tmp_path / "plain" / "0.npy").shape == (96, 192)
    got = np.load(tmp_path / "scene" / "0.npy")
    assert got.shape == (150, 300) and got.dtype == np.float32
    assert sorted(p.name for p in (tmp_path / "scene").iterdir()) == sorted(
        p.name for p in (tmp_path / "plain").iterdir())
    assert np.asarray(Image.open(tmp_path / "scene" / "0.png")).shape[:2] == (150, 300)
    left, right = P.load_images(*P.sceneflow_names(f"{tmp_path}/", "S/left/0001.png\n")[:2])
    want = _model().forward_scene(left, right, tile=(96, 192), tile_batch=2, **KW)
    assert np.array_equal(got, want.disp.cpu().numpy())
    # the other flags keep their file names, at the scene's size
    assert P.main(base + flags + [f"--save_path={tmp_path}/all/", "--lr_check=1", "--confidence=peak"]) == 0
    for name in ("0_right.npy", "0_filled.npy", "0_conf.npy", "0_local.npy"):
        assert np.load(tmp_path / "all" / name).shape == (150, 300), name
    assert np.asarray(Image.open(tmp_path / "all" / "0_occ.png")).shape == (150, 300)
    assert np.array_equal(np.load(tmp_path / "all" / "0.npy"), got)
    with pytest.raises(NotImplementedError, match="photo_check"):
        P.main(base + flags + [f"--save_path={tmp_path}/photo/", "--photo_check"])


def test_predict_cli_satellite_scene(tmp_path):
    """The satellite loop with --scene 1 on a 150 x 300 pair: <name>.png, <name>_in.png,
    <name>_occ.png and <name>_conf.png keep their names and have the image's size; the state
    map is forward_scene's."""
    from PIL import Image
    from leastereo_amd import predict as P
    g = golden("c1_sceneflow")
    d = tmp_path / "sat" / "tile_01"
    d.mkdir(parents=True)
    Image.fromarray(g["left_u8"][:150, :300]).save(d / "satiml.png")
    Image.fromarray(g["right_u8"][:150, :300]).save(d / "satimr.png")
    (tmp_path / "list.txt").write_text("tile_01\n")
    torch.save({"state_dict": state_dict()}, tmp_path / "ckpt.pth")
    (tmp_path / "out").mkdir()
    assert P.main(["--satellite=1", f"--maxdisp={MD}", "--crop_height=96", "--crop_width=192",
                   f"--data_path={tmp_path}/sat/", f"--test_list={tmp_path}/list.txt",
                   f"--resume={tmp_path}/ckpt.pth", f"--save_path={tmp_path}/out/", "--scene=1",
                   "--scene_context=8", "--scene_ramp=8", "--lr_check=1", "--confidence=entropy"]) == 0
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == [
        "tile_01.png", "tile_01_conf.png", "tile_01_in.png", "tile_01_occ.png"]
    for name in ("tile_01.png", "tile_01_conf.png", "tile_01_in.png", "tile_01_occ.png"):
        assert np.asarray(Image.open(tmp_path / "out" / name)).shape[:2] == (150, 300), name
    want = _model().forward_scene(*P.load_images(d / "satiml.png", d / "satimr.png"), tile=(96, 192),
                                  lr_threshold=1.0, confidence=True, **KW)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "tile_01_occ.png")),
                          P.occlusion_u8(want.state.cpu().numpy()))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "tile_01.png")),
                          P.float_to_u8(want.disp.cpu().numpy()))
