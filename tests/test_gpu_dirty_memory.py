"""Every op against recycled memory: the same bits from poisoned buffers, guards intact.

Each case builds its inputs, runs once on plain allocations and then under
``tests/dirty_memory.dirty`` with the patterns 0x00, 0xFF (NaN / -1) and 0x55 (1.5e13 / large
ints), where every ``torch.empty`` / ``empty_like`` / ``new_empty`` of the library returns a
poisoned block between two 4096-byte guards.  Asserted per case: the kernel name or route is the
same in all four runs, every returned tensor is bit-identical in all four (integer views, NaN
equals NaN), and no guard byte changed.  A tensor named ``pattern/...`` is the part of a dirty
allocation beside an ``out=`` channel slice: it must still hold the pattern.  The fp32 conv paths
are also held to the float64 judge of tests/f32_judge.py at that file's bar; the clean run's
correctness otherwise rests on the tests the shapes are taken from.

Regions documented as not written (``UNDEFINED``) are cut off before the comparison; the guards
around them still count.

Workspaces and optional / integer outputs: where each is first written, read from the code before
the first run on poisoned memory (an index read from unwritten memory would be a wild address).
No read precedes the listed write on the stream.

  file                 buffer                      first written                      first read
  speckle.hip          parent (labels), count      speckle_local :184-185, every      speckle_merge :212 (parent),
                       (sizes), 8 n bytes          in-image pixel of every tile       speckle_flatten :251 (count)
  pointcloud.hip       blocks [B][grid.x]          pc_count :151, thread 0 of every   pc_scan :167 (k < nblk only),
                                                   block                              rewritten :188, pc_scatter :225
  pointcloud.hip       count [B]                   pc_scan :193                       never (output)
  forward_warp.hip     key (LDS, one per target)   forward_warp_rows :140, cleared    :171 after the atomicMax at
                                                   before any offer                   :150 / :163
  tile_blend.hip       uncovered (the caller's     blend_clear_kernel :66, launched   tile_blend_kernel :144
                       count)                      at :176 before the blend :200      (atomicAdd)
  evalio.hip           sums (crop)                 hipMemsetAsync :468                u8_stats_kernel (atomics) :475
  evalio.hip           sums, n_valid (train,       train_clear_kernel :179-181,       u8_stats_kernel :526 / :574,
                       tiles)                      launched :518 / :566               atomicAdd :267
  evalio.hip           metric partial [B][G][8]    metrics_partial_kernel :412, all   metrics_final_kernel :423
                                                   8 fields of every (b, block)       (G rows, the launched grid)
  lr_check.hip         none (state / filled are    lr_check_rows, one wave per row    --
                       outputs, null when absent)
  disparity_stats.hip  none (entropy / peak /      the stats kernels :211-227, null   --
                       local outputs)              pointers skipped
  refine.hip           wh, wv, num, den            fgs_init :279                      fgs_transpose :284 / :290
  refine.hip           wht, numt, dent             fgs_transpose :284 / :290          fgs_sweep :292
  refine.hip           cp (q planes)               fgs_col_forward :133, every row    fgs_col_load :186, the same
                                                   of the lane's column               lane, rows clamped to < H
  edge_loss.hip        partial [nblk][4]           reduce4_block (reduce4.h:26),      reduce4_final_kernel
                                                   every block, launched :195         (reduce4.h:37), launched :197
  photometric.hip      partial [nblk][4]           reduce4_block :198 (reduce4.h:26)  reduce4_final_kernel :398
  head.hip             tapsum workspace            tapsum_dpass_c8 :448 /             hwpass :451 / :461 (the fused
                                                   tapsum_dpass_f32 :456-458          kernels :435-442 do not use it)
  conv3d_grad.hip      wgrad part [np][n]          wgrad_kernel :169, launched :543   sum_partials_stage1 :187
  conv3d_grad.hip      wgrad part2 [G][n]          sum_partials_stage1 :551           sum_partials_stage2 :554
  conv3d_grad.hip      BN part [C][slices][2]      bn_moments_kernel :271-272         bn_*_finalize :285 / :334
  conv3d_grad.hip      BN coef                     bn_bwd_finalize_kernel :638        bn_bwd_apply_kernel :642
  conv3d_grad.hip      interpolate-backward gw,    interp_t_kernel :664 / :667        the next interp_t_kernel
                       gh                                                             :667 / :670

What the reading cannot show -- that a grid covers every slot it is meant to -- is what the runs
below show: a slot the grid misses holds the pattern, and the result differs between patterns.
"""
import functools

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels
from tests import dirty_memory as dm
from tests import f32_judge as J

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Regions documented as not written, with the line that says so.  A case cuts them off (and names
# the entry it uses) before it returns its tensors.
UNDEFINED = {
    "pointcloud_rows": "rows at and beyond min(count, capacity) of xyz / rgb / index / normals: "
                       "include/leastereo_hip.h:539, leastereo_amd/kernels.py:1068",
    "dp_down2_only_out": "the `out` of conv3d_bnrelu_wino_dp_down2(only=True) is read, never written: "
                         "leastereo_amd/kernels.py:1982",
}

# Public functions of kernels.py / training.py that allocate and have no case of their own, with
# the reason (tests/test_dirty_memory_cpu.py holds every other one to the table below).
EXEMPT = {}

CASES = {}    # id -> (the wrappers the case runs, factory); factory() -> run; run() -> (route, {name: tensor})


def case(cid, *covers):
    def deco(fn):
        assert cid not in CASES, cid
        CASES[cid] = (covers, fn)
        return fn
    return deco


def covered():
    """Every ``module.function`` some case runs (the coverage guard on the CPU reads this)."""
    return {c for covers, _ in CASES.values() for c in covers}


# ------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape, s=1.0):
    return (torch.randn(shape, generator=g) * s).to(DEV)


def _affine(g, c):
    """scale in [0.5, 1.5), shift N(0, 0.3): some outputs negative, so the ReLU matters."""
    return (torch.rand(c, generator=g) + 0.5).to(DEV), (torch.randn(c, generator=g) * 0.3).to(DEV)


def _w3(g, cout, cin, k=3):
    return (torch.randn(cout, cin, k, k, k, generator=g) / np.sqrt(cin * k ** 3)).to(DEV)


def _w2(g, cout, cin):
    return (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(cin * 9)).to(DEV)


def _u8(seed, *shape):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).to(DEV)


def _slice_of_new(shape, c0, c1, c8=False):
    """A tensor from the allocator (poisoned inside a dirty block) with ``c1`` extra channels
    (blocks, with c8) before and after; returns (the slice, {name: neighbour})."""
    shape = tuple(shape)
    big = torch.empty((shape[0], shape[1] + c0 + c1) + shape[2:], device=DEV,
                      dtype=torch.bfloat16 if c8 else torch.float32)
    return big[:, c0:c0 + shape[1]], {"pattern/before": big[:, :c0], "pattern/after": big[:, c0 + shape[1]:]}


# ------------------------------------------------------------------------------------ fp32 conv paths
def _path_case(path):
    from tests.f32_paths import PATHS
    key, model, entry, settings, _, _, opts = PATHS[path]

    def factory():
        j = J.judged(key, *J.INPUT_SETS[0])

        def run():
            with _lib.tuning(**dict(settings)):
                name, y = entry(j, **opts)
            return name, {"y": y}

        def judge(got):
            e, _ = j.error(got["y"].cpu().numpy())
            assert e <= j.bar(model), (path, e, j.bar(model))
        run.judge = judge
        return run
    return factory


def _register_paths():
    from tests.f32_paths import PATHS
    for path in sorted(PATHS):
        entry = PATHS[path][2].__name__
        covers = (("kernels.conv3d_bnrelu", "kernels.pack_conv_weight") if entry == "_direct" else
                  ("kernels.conv3d_bnrelu_wino", "kernels.pack_conv_weight_wino"))
        CASES["f32/" + path] = (covers, _path_case(path))


_register_paths()

# engine family -> (batch, cin, cout, volume, tuning settings): one ragged volume each, from
# test_gpu_wino.py::test_wino_every_tile (W = 45), f32_judge.TUPLES["c32x32"] (W = 36: whole 16-byte
# rows, partial tiles) and test_gpu_wino44_narrow.py case "a"
ENGINES = {
    "direct": (2, 32, 16, (5, 11, 45), {}),
    "wino1d": (2, 32, 16, (5, 11, 45), {"lea_conv3d_wino_set_tile_override": (1, 2, 2)}),
    "wino2p": (1, 32, 32, (5, 9, 36), {"lea_conv3d_wino44_set": 0}),
    "wino44": (1, 32, 32, (5, 6, 20), {"lea_conv3d_wino44_set": 1}),
}
ENGINE_MODES = ("plain", "affine", "x2", "res", "acc_slice")


def _engine_case(engine, mode):
    b, cin, cout, vol, settings = ENGINES[engine]

    def factory():
        g = _gen(cin * 7 + cout + vol[2])
        x, w = _rn(g, b, cin, *vol), _w3(g, cout, cin)
        scale, shift = _affine(g, cout)
        res = _rn(g, b, cout, *vol)
        xa, xb = x[:, :cin // 2].contiguous(), x[:, cin // 2:].contiguous()
        judge64 = torch.nn.functional.conv3d(x.double().cpu(), w.double().cpu(), None, 1, 1)

        def run():
            with _lib.tuning(**settings):
                if engine == "direct":
                    name = kernels.conv_kernel_name(b, cout, *vol, 3, cin=cin)
                    packed = kernels.pack_conv_weight(w)
                    conv = lambda x, *a, **kw: kernels.conv3d_bnrelu(x, packed, cout, 3, *a, **kw)  # noqa: E731
                else:
                    name = kernels.wino_kernel_name(b, cout, *vol, cin=cin)
                    packed = kernels.pack_conv_weight_wino(w)
                    conv = lambda x, *a, **kw: kernels.conv3d_bnrelu_wino(x, packed, cout, *a, **kw)  # noqa: E731
                extra = {}
                if mode == "plain":
                    y = conv(x, None, None, relu=False)
                elif mode == "affine":
                    y = conv(x, scale, shift, relu=True)
                elif mode == "x2":
                    y = conv(xa, None, None, relu=False, x2=xb)
                elif mode == "res":
                    y = conv(x, scale, shift, relu=True, residual=res)
                else:  # accumulate into a channel slice of a tensor from the allocator
                    out, extra = _slice_of_new((b, cout) + vol, 3, 5)
                    out.copy_(res)
                    y = conv(x, scale, shift, relu=True, out=out, accumulate=True)
            return name, dict(extra, y=y, packed=packed)

        def judge(got):  # the float64 link, at the bar of the tests the volume is taken from
            want = judge64
            if mode in ("affine", "res", "acc_slice"):
                want = (want * scale.double().cpu().view(1, -1, 1, 1, 1) + shift.double().cpu().view(1, -1, 1, 1, 1)).relu()
            if mode in ("res", "acc_slice"):
                want = want + res.double().cpu()
            np.testing.assert_allclose(got["y"].double().cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-4)
        run.judge = judge
        return run
    return factory


for _e in ENGINES:
    for _m in ENGINE_MODES:
        CASES[f"engine/{_e}/{_m}"] = (
            ("kernels.conv3d_bnrelu", "kernels.pack_conv_weight") if _e == "direct" else
            ("kernels.conv3d_bnrelu_wino", "kernels.pack_conv_weight_wino"), _engine_case(_e, _m))


# ------------------------------------------------------------------------------------ packers, compared whole
@case("pack/conv3d", "kernels.pack_conv_weight")
def _():
    g = _gen(1)
    ws = [_w3(g, co, ci, k) for co, ci, k in [(16, 32, 3), (5, 16, 3), (1, 16, 3), (24, 12, 3), (32, 128, 1),
                                               (80, 4, 3), (24, 64, 1)]]
    return lambda: (None, {str(tuple(w.shape)): kernels.pack_conv_weight(w) for w in ws})


@case("pack/wino", "kernels.pack_conv_weight_wino")
def _():
    g = _gen(2)
    ws = [_w3(g, co, ci) for co, ci in [(16, 16), (32, 32), (24, 8), (48, 16), (64, 128), (96, 32), (8, 8), (4, 8),
                                        (6, 4), (20, 12)]]

    def run():
        out = {}
        for mode in (0, 1, 2, 3):  # the F(4,3) x F(4,3) layouts beside the default ones
            with _lib.tuning(lea_conv3d_wino44_set=mode):
                for w in ws:
                    out[f"{tuple(w.shape)} w44={mode}"] = kernels.pack_conv_weight_wino(w)
        return None, out
    return run


@case("pack/conv2d", "kernels.pack_conv2d_weight")
def _():
    g = _gen(3)
    ws = [_w2(g, co, ci) for co, ci in [(5, 3), (16, 4), (32, 3), (16, 5), (48, 64), (192, 32), (24, 9), (8, 13)]]
    return lambda: (None, {str(tuple(w.shape)): kernels.pack_conv2d_weight(w) for w in ws})


@case("pack/conv2d_windowed", "kernels.pack_conv2d_weight")
def _():
    g = _gen(4)
    w = _w2(g, 72, 4)
    return lambda: (None, {f"split{s}": kernels.pack_conv2d_weight_windowed(w, s) for s in (0, 24, 40)})


@case("pack/bf16", "kernels.pack_conv_weight_bf16", "kernels.pack_conv2d_weight_bf16")
def _():
    g = _gen(5)
    w3 = [_w3(g, co, ci, k) for co, ci, k in [(8, 8, 3), (32, 16, 3), (96, 64, 3), (8, 24, 1), (64, 128, 1), (24, 8, 3)]]
    w2 = [_w2(g, co, ci) for co, ci in [(8, 8), (96, 16), (16, 32)]]

    def run():
        out = {str(tuple(w.shape)): kernels.pack_conv_weight_bf16(w) for w in w3}
        out.update({str(tuple(w.shape)): kernels.pack_conv2d_weight_bf16(w) for w in w2})
        return None, out
    return run


@case("pack/cv_stem_split", "kernels.cv_stem_split_weights")
def _():
    g = _gen(6)
    ws = [_w3(g, co, 2 * c) for co, c in [(16, 4), (8, 16), (24, 8)]]

    def run():
        out = {}
        for w in ws:
            out[f"{tuple(w.shape)} wl"], out[f"{tuple(w.shape)} wr"] = kernels.cv_stem_split_weights(w)
        return None, out
    return run


# ------------------------------------------------------------------------------------ fused and level-changing convs
@case("fused/resampled", "kernels.conv3d_bnrelu_resampled")
def _():
    g = _gen(7)
    x = _rn(g, 2, 16, 4, 6, 10)
    size = (7, 11, 19)
    w1, w3 = _w3(g, 16, 16, 1), _w3(g, 16, 16, 3)
    scale, shift = _affine(g, 16)
    res = _rn(g, 2, 16, *size)

    def run():
        p1, p3 = kernels.pack_conv_weight(w1), kernels.pack_conv_weight(w3)
        names = (kernels.conv_kernel_name(2, 16, *size, 1, True, 16), kernels.conv_kernel_name(2, 16, *size, 3, True, 16))
        out, extra = _slice_of_new((2, 16) + size, 2, 3)
        out.copy_(res)
        return names, dict(extra, k1=kernels.conv3d_bnrelu_resampled(x, size, p1, 16, 1, scale, shift),
                           k3=kernels.conv3d_bnrelu_resampled(x, size, p3, 16, 3, None, None, relu=False),
                           acc=kernels.conv3d_bnrelu_resampled(x, size, p1, 16, 1, scale, shift, out=out,
                                                               accumulate=True))
    return run


@case("fused/conv1x1_heads", "kernels.conv1x1_heads")
def _():
    g = _gen(8)  # test_gpu_conv1x1_heads.py HEADS[0] on VOLUMES[0]
    b, cin, ca, cb, vol = 1, 64, 16, 8, (3, 5, 7)
    x = _rn(g, b, cin, *vol)
    w = _w3(g, ca + cb, cin, 1)
    sa, ha = _affine(g, ca)

    def run():
        packed = kernels.pack_conv_weight(w)
        name = kernels._decode(_lib.load().lea_conv1x1_heads_kernel_name(b, ca + cb, *vol))
        ya, yb = kernels.conv1x1_heads(x, packed, ca, sa, ha, True, cb, None, None, False)
        oa, ea = _slice_of_new((b, ca) + vol, 1, 2)
        ob, eb = _slice_of_new((b, cb) + vol, 2, 1)
        kernels.conv1x1_heads(x[:, :32], packed, ca, sa, ha, True, cb, None, None, False, out_a=oa, out_b=ob,
                              x2=x[:, 32:])
        extra = {k + "/a": v for k, v in ea.items()}
        extra.update({k + "/b": v for k, v in eb.items()})
        return name, dict(extra, ya=ya, yb=yb, oa=oa, ob=ob)
    return run


@case("fused/costvolume", "kernels.conv3d_bnrelu_costvolume", "kernels.conv3d_bnrelu_costvolume_wino")
def _():
    g = _gen(9)  # test_gpu_wino.py costvolume row (2, 16, 16, 27, (5, 19))
    b, c, cout, md, hw = 2, 16, 16, 27, (5, 19)
    fl, fr = _rn(g, b, c, *hw), _rn(g, b, c, *hw)
    w = _w3(g, cout, 2 * c)
    scale, shift = _affine(g, cout)

    def run():
        names = (kernels.costvolume_kernel_name(b, cout, md // 3, *hw),
                 kernels.wino_kernel_name(b, cout, md // 3, *hw, True, cin=2 * c))
        return names, {
            "f32": kernels.conv3d_bnrelu_costvolume(fl, fr, md, kernels.pack_conv_weight(w), cout, scale, shift),
            "wino": kernels.conv3d_bnrelu_costvolume_wino(fl, fr, md, kernels.pack_conv_weight_wino(w), cout, scale,
                                                          shift)}
    return run


@case("fused/wino_down2", "kernels.conv3d_bnrelu_wino_down2", "kernels.conv3d_bnrelu_wino_down2_cat")
def _():
    g = _gen(10)  # the first rows of test_gpu_down2.py / test_gpu_down2_cells.py, and a partial W tile
    rows = [(1, 32, 0, 32, (4, 2, 32)), (2, 12, 0, 32, (12, 6, 40)), (1, 16, 16, 32, (4, 2, 32))]
    ops = []
    for b, c1, c2, cout, vol in rows:
        ops.append((_rn(g, b, c1, *vol), _rn(g, b, c2, *vol) if c2 else None, _w3(g, cout, c1 + c2), _affine(g, cout)))

    def run():
        names, out = [], {}
        for (b, c1, c2, cout, vol), (x, x2, w, (sc, sh)) in zip(rows, ops):
            names.append(kernels.wino_down2_kernel_name(b, c1 + c2, cout, *vol, c2))
            packed = kernels.pack_conv_weight_wino(w)
            out[str((b, c1, c2, vol))] = (kernels.conv3d_bnrelu_wino_down2(x, packed, cout, sc, sh) if x2 is None else
                                          kernels.conv3d_bnrelu_wino_down2_cat(x, x2, packed, cout, sc, sh))
        return tuple(names), out
    return run


@case("fused/wino_dp_down2", "kernels.conv3d_bnrelu_wino_dp_down2")
def _():
    g = _gen(11)  # DP_SHAPES[0] and the partial W tile of DP_SHAPES[2] (test_gpu_down2_cells.py)
    rows = [(1, 8, 8, (2, 4, 64)), (2, 8, 8, (6, 4, 96))]
    ops = [(_rn(g, b, cin, *vol), _w3(g, cout, cin), _affine(g, cout), _rn(g, b, cout, *vol))
           for b, cin, cout, vol in rows]

    def run():
        names, out = [], {}
        for (b, cin, cout, vol), (x, w, (sc, sh), part) in zip(rows, ops):
            half = tuple(n // 2 for n in vol)
            packed = kernels.pack_conv_weight_wino(w)
            for only in (False, True):
                names.append(kernels.wino_dp_down2_kernel_name(b, cin, cout, *vol, only))
                y, ey = _slice_of_new((b, cout) + vol, 8, 8)
                y.copy_(part)
                down, ed = _slice_of_new((b, cout) + half, 0, 8)
                kernels.conv3d_bnrelu_wino_dp_down2(x, packed, cout, sc, sh, True, y, down, accumulate=True, only=only)
                tag = f"{vol} only={only}"
                out[tag + " down"] = down
                out[tag + " out"] = y  # side: the plain launch's output; only: the partial sums, as they were
                out.update({f"{k}/{tag}/out": v for k, v in ey.items()})
                out.update({f"{k}/{tag}/down": v for k, v in ed.items() if v.numel()})
            # only=True without a residual: there is no `out` at all (UNDEFINED["dp_down2_only_out"])
            down = torch.empty((b, cout) + half, device=DEV)
            out[f"{vol} only, no out"] = kernels.conv3d_bnrelu_wino_dp_down2(x, packed, cout, sc, sh, True, None, down,
                                                                            only=True)
        return tuple(names), out
    return run


@case("fused/resample", "kernels.resample_trilinear")
def _():
    g = _gen(12)
    x = _rn(g, 2, 5, 3, 5, 7)[:, 1:4]  # a channel slice
    scale, shift = _affine(g, 3)
    sizes = [(6, 10, 14), (5, 9, 13), (2, 3, 4), (3, 5, 21)]

    def run():
        out = {}
        for size in sizes:
            for ac in (True, False):
                out[f"{size} ac={ac}"] = kernels.resample_trilinear(x, size, ac)
                out[f"{size} ac={ac} affine"] = kernels.resample_trilinear(x, size, ac, None, scale, shift, True)
        y, extra = _slice_of_new((2, 3) + sizes[1], 2, 1)
        out["slice"] = kernels.resample_trilinear(x, sizes[1], True, y, scale, shift, True)
        return None, dict(extra, **out)
    return run


@case("fused/resample_down2", "kernels.resample_trilinear_down2")
def _():
    g = _gen(13)  # test_gpu_down2_cells.py: the first two rows
    rows = [(1, 8, (2, 2, 8)), (2, 8, (3, 5, 12))]
    ops = [(_rn(g, b, c + 2, *vol)[:, 1:c + 1], _affine(g, c)) for b, c, vol in rows]

    def run():
        out = {}
        for (b, c, vol), (z, (sc, sh)) in zip(rows, ops):
            up = tuple(2 * n for n in vol)
            out[f"{vol} y"], out[f"{vol} y2"] = kernels.resample_trilinear_down2(z, up)
            y, ey = _slice_of_new((b, c) + up, 0, 1)
            d, ed = _slice_of_new((b, c) + vol, 1, 0)
            kernels.resample_trilinear_down2(z, up, y, d, sc, sh, True)
            out[f"{vol} y affine"], out[f"{vol} y2 affine"] = y, d
            out[f"pattern/{vol}/y"], out[f"pattern/{vol}/y2"] = ey["pattern/after"], ed["pattern/before"]
        return None, out
    return run


@case("fused/tapsum", "kernels.tapsum_upsample")
def _():
    g = _gen(14)
    q1, q2 = _rn(g, 1, 27, 4, 5, 6), _rn(g, 2, 54, 3, 4, 5)
    scale, shift = _affine(g, 2)

    def run():
        out = {}
        for rows in (2, 0):  # the fused kernel (the default) and the form that goes through the workspace
            with _lib.tuning(lea_tapsum_set_rows=rows):
                out[f"rows{rows} 1"] = kernels.tapsum_upsample(q1, 1, (12, 15, 18))
                out[f"rows{rows} 2"] = kernels.tapsum_upsample(q2, 2, (7, 11, 13), scale, shift, True)
        return None, out
    return run


# ------------------------------------------------------------------------------------ cost volume, factored stem0
@case("cv/build", "kernels.build_cost_volume")
def _():
    g = _gen(15)
    a = (_rn(g, 1, 3, 2, 5), _rn(g, 1, 3, 2, 5))
    b = (_rn(g, 2, 4, 3, 16), _rn(g, 2, 4, 3, 16))
    return lambda: (None, {"(1, 3, 2, 5) D3=10": kernels.build_cost_volume(*a, 30),
                           "(2, 4, 3, 16) D3=8": kernels.build_cost_volume(*b, 24)})


def _cv_case(b, cout, md, h, w, c8):
    """conv2d_bnrelu_windowed -> cv_stem_combine (and _down2) with the maps from the allocator, so
    a read of a column the windowed launch skips shows up (test_gpu_windowed_maps.py SHAPES)."""
    c = 4 if not c8 else 16

    def factory():
        g = _gen(cout + md + h + w)
        d3 = md // 3
        fl, fr = _rn(g, b, c, 1, h, w), _rn(g, b, c, 1, h, w)
        wt = _w3(g, cout, 2 * c)
        scale, shift = _affine(g, cout)

        def run():
            wl, wr = kernels.cv_stem_split_weights(wt)
            out = {}
            if c8:
                flc, frc = kernels.to_c8(fl), kernels.to_c8(fr)
                lm = kernels.conv2d_bnrelu_bf16(flc, kernels.pack_conv2d_weight_bf16(wl), 9 * cout, None, None, False)
                rm = kernels.conv2d_bnrelu_bf16(frc, kernels.pack_conv2d_weight_bf16(wr), 6 * cout, None, None, False)
                out["y"] = kernels.cv_stem_combine(lm, rm, cout, d3, scale, shift, True)
                return None, out
            wlt = wl.view(3, 3, cout, c, 3, 3).transpose(0, 1).reshape(wl.shape)
            lwin, rwin = kernels.cv_stem_map_windows(d3, w)
            lm = kernels.conv2d_bnrelu_windowed(fl, kernels.pack_conv2d_weight_windowed(wlt, 3 * cout), 9 * cout,
                                                3 * cout, (lwin,))
            rm = kernels.conv2d_bnrelu_windowed(fr, kernels.pack_conv2d_weight_windowed(wr, 3 * cout), 6 * cout,
                                                3 * cout, rwin)
            out["y"] = kernels.cv_stem_combine(lm, rm, cout, d3, scale, shift, True, tmajor=True)
            if kernels.cv_stem_down2_supported(lm, cout, d3):
                out["down2 y"], out["down2 y2"] = kernels.cv_stem_combine_down2(lm, rm, cout, d3, scale, shift, True,
                                                                               tmajor=True)
            # the maps themselves: only where the windowed launch writes (its docstring: nothing else of
            # `out` is written), so the columns outside the windows must still hold the pattern
            for name, m, windows in (("lmaps", lm, [lwin]), ("rmaps", rm, list(rwin))):
                inside = torch.zeros(w, dtype=torch.bool, device=DEV)
                for s, e in kernels.conv2d_windowed_tiles(w, windows):
                    inside[16 * s:16 * e] = True
                out[name + " all columns"] = m[:, :3 * cout]
                out[name + " windows"] = m[:, 3 * cout:][..., inside]
                if bool((~inside).any()):
                    out["pattern/" + name] = m[:, 3 * cout:][..., ~inside]
            return (lwin, rwin, kernels.cv_stem_down2_supported(lm, cout, d3)), out
        return run
    return factory


CASES["cv/stem_f32/8x24x6x64"] = (("kernels.conv2d_bnrelu_windowed", "kernels.cv_stem_combine",
                                   "kernels.cv_stem_combine_down2"), _cv_case(1, 8, 24, 6, 64, False))
CASES["cv/stem_f32/16x24x6x36_b2"] = (("kernels.conv2d_bnrelu_windowed", "kernels.cv_stem_combine",
                                       "kernels.cv_stem_combine_down2"), _cv_case(2, 16, 24, 6, 36, False))
CASES["cv/stem_c8/16x27x5x19"] = (("kernels.cv_stem_combine",), _cv_case(2, 16, 27, 5, 19, True))


# ------------------------------------------------------------------------------------ 2D feature ops
@case("feature/conv2d", "kernels.conv2d_bnrelu")
def _():
    g = _gen(16)
    # the few-channel tile (feature_judge.SMALL) and the 2D DMA engine (DMA2D), ragged H and W
    rows = [(2, 3, 5, (9, 35)), (2, 5, 20, (9, 35)), (1, 32, 32, (9, 36)), (1, 64, 48, (9, 35))]
    ops = [(_rn(g, b, cin, 1, *hw), _w2(g, cout, cin), _affine(g, cout), _rn(g, b, cout, 1, *hw))
           for b, cin, cout, hw in rows]

    def run():
        names, out = [], {}
        for (b, cin, cout, hw), (x, w, (sc, sh), res) in zip(rows, ops):
            names.append(kernels.conv2d_kernel_name(b, cout, *hw, cin))
            p = kernels.pack_conv2d_weight(w)
            tag = f"{cin}->{cout}"
            out[tag] = kernels.conv2d_bnrelu(x, p, cout, None, None, relu=False)
            out[tag + " res"] = kernels.conv2d_bnrelu(x, p, cout, sc, sh, True, residual=res)
            y, extra = _slice_of_new((b, cout, 1) + hw, 1, 2)
            y.copy_(res)
            out[tag + " acc"] = kernels.conv2d_bnrelu(x, p, cout, sc, sh, True, out=y, accumulate=True)
            out.update({f"{k}/{tag}": v for k, v in extra.items()})
        return tuple(names), out
    return run


@case("feature/conv2d_pair", "kernels.conv2d_bnrelu_pair")
def _():
    g = _gen(17)  # feature_judge.PAIR: the first row and a ragged one
    rows = [(8, 8, 16), (5, 8, 32)]
    hw = (9, 35)
    ops = [(_rn(g, 2, cin, 1, *hw), _w2(g, cout, cin), _affine(g, cout), _rn(g, 2, c1, 1, *hw)) for cin, c1, cout in rows]

    def run():
        out = {}
        for (cin, c1, cout), (x, w, (sc, sh), res) in zip(rows, ops):
            p = kernels.pack_conv2d_weight(w)
            big = torch.empty((2, cout + 3, 1) + hw, device=DEV)  # two non-adjacent slots of a cat buffer
            o1, o2 = big[:, :c1], big[:, c1 + 3:]
            kernels.conv2d_bnrelu_pair(x, p, c1, cout, sc, sh, True, o1, o2, residual=res)
            out[f"{cin} o1"], out[f"{cin} o2"], out[f"pattern/{cin}"] = o1, o2, big[:, c1:c1 + 3]
        return None, out
    return run


@case("feature/conv2d_s3", "kernels.conv2d_s3_bnrelu")
def _():
    g = _gen(18)
    x, w = _rn(g, 1, 5, 1, 31, 46), _w2(g, 20, 5)
    x2, w2 = _rn(g, 2, 16, 1, 22, 198), _w2(g, 32, 16)
    sc, sh = _affine(g, 20)
    return lambda: (None, {"(1, 5, 20, (31, 46))": kernels.conv2d_s3_bnrelu(x, w, sc, sh),
                           "(2, 16, 32, (22, 198))": kernels.conv2d_s3_bnrelu(x2, w2, None, None, False)})


@case("feature/stem", "kernels.feature_stem")
def _():
    g = _gen(19)  # feature_judge.STEM_SHAPES
    w0, w1 = _w2(g, 16, 3), _w2(g, 32, 16)
    a0, a1 = _affine(g, 16), _affine(g, 32)
    xs = {hw: (_rn(g, 1, 3, *hw), _rn(g, 1, 3, *hw), _rn(g, 2, 3, *hw)) for hw in [(5, 7), (23, 200)]}

    def run():
        out = {}
        for hw, (l, r, two) in xs.items():
            for c8 in (False, True):
                tag = f"{hw} {'c8' if c8 else 'f32'}"
                out[tag + " pair"] = kernels.feature_stem(l, w0, *a0, w1, *a1, c8=c8, x2=r)
                out[tag + " b2"] = kernels.feature_stem(two, w0, *a0, w1, *a1, c8=c8)
                out[tag + " b2 pair"] = kernels.feature_stem(two, w0, *a0, w1, *a1, c8=c8, x2=two.flip(0))
        return None, out
    return run


# ------------------------------------------------------------------------------------ bf16
def _bf(t):
    """Values that bf16 holds exactly."""
    return t.to(torch.bfloat16).float()


@case("bf16/layout", "kernels.to_c8", "kernels.from_c8")
def _():
    g = _gen(20)
    x5, x4 = _rn(g, 2, 24, 3, 5, 7)[:, 8:], _rn(g, 1, 8, 5, 19)

    def run():
        c5, c4 = kernels.to_c8(x5), kernels.to_c8(x4)
        return None, {"c5": c5, "c4": c4, "f5": kernels.from_c8(c5), "f4": kernels.from_c8(c4)}
    return run


@case("bf16/conv3d", "kernels.conv3d_bnrelu_bf16")
def _():
    g = _gen(21)  # the first rows of test_gpu_bf16_exact.py: VOL_A tiles, the planner's stream kernel, 1x1
    vol_a, vol_s = (5, 19, 37), (5, 9, 20)
    rows = {  # tag: (cin, cout, k, volume, settings, second source's channels)
        "tile": (16, 32, 3, vol_a, {"lea_conv3d_bf16_set_tile_override": (8, 2, 1)}, 0),
        "tile x2": (64, 96, 3, vol_a, {"lea_conv3d_bf16_set_tile_override": (4, 1, 2)}, 32),
        "stream": (16, 16, 3, vol_s, {}, 0),
        "1x1 stream": (24, 8, 1, vol_a, {}, 0),
        "1x1 tile": (24, 8, 1, vol_a, {"lea_conv3d_bf16_set_stream1x1": 0,
                                      "lea_conv3d_bf16_set_tile_override": (8, 1, 1)}, 0),
    }
    ops = {}
    for tag, (cin, cout, k, vol, _, _) in rows.items():
        ops[tag] = (kernels.to_c8(_bf(_rn(g, 2, cin, *vol))), _bf(_w3(g, cout, cin, k)), _affine(g, cout),
                    kernels.to_c8(_bf(_rn(g, 2, cout, *vol))))
    torch.cuda.synchronize()

    def run():
        names, out = [], {}
        for tag, (cin, cout, k, vol, settings, cin2) in rows.items():
            xc, w, (sc, sh), rc = ops[tag]
            with _lib.tuning(**settings):
                names.append(kernels.conv_kernel_name_bf16(2, cout, cin, *vol, k, cin2=cin2))
                packed = kernels.pack_conv_weight_bf16(w)
                x1, x2 = (xc[:, :-(cin2 // 8)], xc[:, -(cin2 // 8):]) if cin2 else (xc, None)
                out[tag] = kernels.conv3d_bnrelu_bf16(x1, packed, cout, k, sc, sh, True, x2=x2)
                out[tag + " res"] = kernels.conv3d_bnrelu_bf16(x1, packed, cout, k, sc, sh, True, x2=x2, residual=rc)
                y, extra = _slice_of_new((2, cout // 8) + vol + (8,), 1, 1, c8=True)
                y.copy_(rc)
                out[tag + " acc"] = kernels.conv3d_bnrelu_bf16(x1, packed, cout, k, sc, sh, False, out=y,
                                                               accumulate=True, x2=x2)
                out.update({f"{k_}/{tag}": v for k_, v in extra.items()})
        return tuple(names), out
    return run


@case("bf16/pair_sum", "kernels.conv3d_bnrelu_bf16")
def _():
    g = _gen(22)  # test_pair_launch_rounds_as_its_kernel: c 8 on (4, 4, 16), c 16 on (9, 12, 33)
    rows = [(8, (4, 4, 16)), (16, (9, 12, 33))]
    ops = [(kernels.to_c8(_bf(_rn(g, 2, c, *vol))), kernels.to_c8(_bf(_rn(g, 2, c, *vol))), _bf(_w3(g, c, c)),
            _bf(_w3(g, c, c)), _affine(g, 2 * c)) for c, vol in rows]

    def run():
        out = {}
        for (c, vol), (xa, xb, wa, wb, (sc, sh)) in zip(rows, ops):
            packed = torch.cat([kernels.pack_conv_weight_bf16(wa), kernels.pack_conv_weight_bf16(wb)])
            for split in (0, 1):
                with _lib.tuning(lea_conv3d_bf16_set_pair_split=split):
                    y, extra = _slice_of_new((2, c // 8) + vol + (8,), 1, 1, c8=True)
                    assert kernels.pair_sum_supported_bf16(xa, xb, y)
                    out[f"c{c} split{split}"] = kernels.conv3d_bnrelu_bf16(xa, packed, c, 3, sc, sh, True, y, x2=xb,
                                                                           pair_sum=True)
                    out.update({f"{k}/c{c} split{split}": v for k, v in extra.items()})
        return None, out
    return run


@case("bf16/resampled_and_heads", "kernels.conv1x1_resampled_bf16", "kernels.resample_trilinear_bf16",
      "kernels.tapsum_upsample_bf16")
def _():
    g = _gen(23)
    x = kernels.to_c8(_bf(_rn(g, 2, 32, 3, 5, 7)))  # the gather-GEMM takes cin % 32, cout % 16
    w = _bf(_w3(g, 32, 32, 1))
    sc, sh = _affine(g, 32)
    s2, h2 = _affine(g, 32)
    q = kernels.to_c8(_bf(_rn(g, 1, 32, 4, 5, 6)))  # 27 channels padded to 32
    size = (5, 9, 13)

    def run():
        packed = kernels.pack_conv_weight_bf16(w)
        out = {"rs1x1": kernels.conv1x1_resampled_bf16(x, size, packed, 32, sc, sh)}
        y, extra = _slice_of_new((2, 4) + size + (8,), 1, 1, c8=True)
        out["rs1x1 slice"] = kernels.conv1x1_resampled_bf16(x, size, packed, 32, sc, sh, False, out=y)
        for ac in (True, False):
            out[f"resample ac={ac}"] = kernels.resample_trilinear_bf16(x, size, ac)
            out[f"resample ac={ac} affine"] = kernels.resample_trilinear_bf16(x, (6, 10, 14), ac, None, s2, h2, True)
        for rows in (2, 0):  # fused, and through the workspace (tapsum_dpass_c8)
            with _lib.tuning(lea_tapsum_set_rows=rows):
                out[f"tapsum rows{rows}"] = kernels.tapsum_upsample_bf16(q, 1, (12, 15, 18))
        return None, dict(extra, **out)
    return run


@case("bf16/conv2d_and_costvolume", "kernels.conv2d_bnrelu_bf16", "kernels.conv3d_bnrelu_costvolume_bf16")
def _():
    g = _gen(24)  # test_gpu_bf16_exact.py: conv2d (8, 8, (19, 33)); costvolume (16, 16, 27, (5, 19))
    x = kernels.to_c8(_bf(_rn(g, 2, 8, 19, 33)))
    w = _bf(_w2(g, 8, 8))
    sc, sh = _affine(g, 8)
    r = kernels.to_c8(_bf(_rn(g, 2, 8, 19, 33)))
    fl, fr = kernels.to_c8(_bf(_rn(g, 2, 16, 5, 19))), kernels.to_c8(_bf(_rn(g, 2, 16, 5, 19)))
    wc = _bf(_w3(g, 16, 32))
    s3, h3 = _affine(g, 16)

    def run():
        p = kernels.pack_conv2d_weight_bf16(w)
        out = {"conv2d": kernels.conv2d_bnrelu_bf16(x, p, 8, sc, sh), "conv2d res": kernels.conv2d_bnrelu_bf16(
            x, p, 8, sc, sh, True, residual=r)}
        y, extra = _slice_of_new((2, 1, 1, 19, 33, 8), 1, 1, c8=True)
        y.copy_(r)
        out["conv2d acc"] = kernels.conv2d_bnrelu_bf16(x, p, 8, sc, sh, True, out=y, accumulate=True)
        name = kernels.conv_kernel_name_bf16(2, 16, 32, 9, 5, 19, 3, True)
        out["costvolume"] = kernels.conv3d_bnrelu_costvolume_bf16(fl, fr, 27, kernels.pack_conv_weight_bf16(wc), 16,
                                                                  s3, h3)
        return name, dict(extra, **out)
    return run


# ------------------------------------------------------------------------------------ heads and post-processing
def _cost(g, b, d3, h3, w3, gain=3.0):
    return _rn(g, b, 1, d3, h3, w3, s=gain)


@case("head/disparity_regression", "kernels.disparity_regression")
def _():
    g = _gen(25)  # test_gpu_f32_numerics.py: the first two shapes of the forms test
    costs = {((1, 1, 16, 7, 4), 48): _cost(g, 1, 16, 7, 4), ((2, 1, 8, 5, 6), 24): _cost(g, 2, 8, 5, 6)}

    def run():
        out = {}
        for (shape, md), c in costs.items():
            for form in (0, 1, 2, 3, 4):
                with _lib.tuning(lea_disparity_set_register_form=form):
                    for fast in (False, True):
                        out[f"{shape} form{form} fast={fast}"] = kernels.disparity_regression(c, md, fast)
        return None, out
    return run


@case("head/stats_right_lr", "kernels.disparity_regression_stats", "kernels.disparity_regression_right",
      "kernels.lr_check")
def _():
    g = _gen(26)
    c = _cost(g, 2, 8, 5, 6)
    dl, dr = _rn(g, 2, 19, 70, s=4.0).abs(), _rn(g, 2, 19, 70, s=4.0).abs()

    def run():
        out = {}
        for fast in (False, True):
            st = kernels.disparity_regression_stats(c, 24, 3, fast)
            out.update({f"stats fast={fast} {n}": getattr(st, n) for n in st._fields})
            out[f"right fast={fast}"] = kernels.disparity_regression_right(c, 24, fast)
        out["stats peak only"] = kernels.disparity_regression_stats(c, 24, 4, False, False, True, False).peak
        lr = kernels.lr_check(dl, dr, 1.0)
        out["lr state"], out["lr filled"] = lr.state, lr.disp_filled
        lr = kernels.lr_check(out["stats fast=False disp"], out["right fast=False"], 1.0)
        out["lr state of the cost"], out["lr filled of the cost"] = lr.state, lr.disp_filled
        return None, out
    return run


@case("post/median_refine_speckle", "kernels.median_blur5", "kernels.fgs_refine", "kernels.speckle_filter")
def _():
    g = _gen(27)
    h, w = 41, 67  # more than one speckle tile (16 x 64) each way, a ragged last one
    disp = (_rn(g, 2, h, w, s=0.4) + torch.linspace(0, 20, w, device=DEV)).contiguous()
    disp[:, 10:14, 20:25] += 9.0   # a speckle
    disp[0, 30, 40] = float("nan")
    guide = torch.rand((2, 3, h, w), generator=g).to(DEV)
    conf = torch.rand((2, h, w), generator=g).to(DEV)
    excl = (torch.rand((2, h, w), generator=g) < 0.05).to(DEV)
    finite = torch.nan_to_num(disp, nan=0.0)

    def run():
        out = {"median 1": kernels.median_blur5(finite, 1), "median 2": kernels.median_blur5(finite[0], 2)}
        out["refined"], out["support"] = kernels.fgs_refine(guide, finite, conf, excl, return_support=True)
        out["refined plain"] = kernels.fgs_refine(guide[:, :1], finite, iterations=1)
        sp = kernels.speckle_filter(disp, excl, max_size=30, want_labels=True)
        out.update({"speckle " + n: getattr(sp, n) for n in ("state", "size", "labels", "filtered")})
        out["speckle state only"] = kernels.speckle_filter(disp[0], None, 30, want_size=False,
                                                           want_filtered=False).state
        return None, out
    return run


@case("post/reproject", "kernels.reproject")
def _():
    from leastereo_amd.pointcloud import q_matrix
    g = _gen(28)
    h, w = 41, 67
    disp = (_rn(g, 2, h, w).abs() * 10 + 1).contiguous()
    disp[:, ::7, ::5] = 0.0  # not valid
    img = _u8(28, 2, h, w, 3)
    excl = (torch.rand((2, h, w), generator=g) < 0.05).to(DEV)
    Q = q_matrix(700.0, 0.12, 33.0, 20.0)

    def run():
        out = {}
        for tag, cap in (("full", None), ("capped", 500)):
            pc = kernels.reproject(disp, Q, img, excl, normals=True, capacity=cap, want_points=True, want_valid=True)
            n = pc.count.clamp(max=pc.xyz.shape[1]).tolist()  # UNDEFINED["pointcloud_rows"]
            out.update({f"{tag} points": pc.points, f"{tag} valid": pc.valid, f"{tag} count": pc.count})
            for name in ("xyz", "rgb", "index", "normals"):
                for i, rows in enumerate(n):
                    out[f"{tag} {name}[{i}]"] = getattr(pc, name)[i, :rows]
        return None, out
    return run


@case("post/rectify", "kernels.rectify_u8")
def _():
    from leastereo_amd import rectify as rc
    g = _gen(29)
    h, w, ho, wo = 30, 45, 41, 67  # odd widths at both pixel strides, an output larger than its source
    maps = torch.stack([torch.rand((1, 2, ho, wo), generator=g) * (w + 8) - 4,
                        torch.rand((1, 2, ho, wo), generator=g) * (h + 8) - 4], 2).to(DEV)
    cam = rc.CameraModel([[40.0, 0, 22.0], [0, 40.0, 15.0], [0, 0, 1]], (0.05, -0.01, 0.001, 0.002))
    calib = rc.stereo_rectify(cam, cam, np.eye(3), np.array([-0.1, 0.0, 0.0]), (h, w)).calib()
    imgs = {ps: (_u8(30 + ps, 2, h, w, ps), _u8(40 + ps, 2, h, w, ps)) for ps in (3, 4)}

    def run():
        out = {}
        for ps, (l, r) in imgs.items():
            a = kernels.rectify_u8(l, r, maps=maps, fill=7, want_maps=True)
            b = kernels.rectify_u8(l, r, calib=calib, size=(ho, wo), want_maps=True)
            for tag, res in (("maps", a), ("calib", b)):
                out.update({f"ps{ps} {tag} {n}": getattr(res, n) for n in res._fields})
        return None, out
    return run


@case("post/forward_warp", "kernels.forward_warp")
def _():
    g = _gen(31)
    h, w = 19, 70
    img = torch.rand((2, 3, h, w), generator=g).to(DEV)
    disp = (_rn(g, 2, h, w, s=0.3) + torch.linspace(2, 12, w, device=DEV)).contiguous()
    disp[:, :, 30:40] += 8.0  # a foreground object: an occlusion and a hole
    excl = (torch.rand((2, h, w), generator=g) < 0.05).to(DEV)
    scale = torch.tensor([1.0, 0.5], device=DEV)

    def run():
        out = {}
        for tag, fill in (("fill", True), ("nofill", False)):
            v = kernels.forward_warp(img, disp, scale, excl, fill=fill, fill_value=-1.0, want_source=True)
            out.update({f"{tag} {n}": getattr(v, n) for n in v._fields})
        return None, out
    return run


# ------------------------------------------------------------------------------------ losses and data
@case("loss/edge", "kernels.edge_loss_sums", "kernels.edge_loss_grad")
def _():
    g = _gen(32)
    b, h, w = 3, 41, 67
    target = (_rn(g, b, h, w, s=6.0) + 20).contiguous()
    target[:, ::9, ::4] = 0.0  # invalid
    pred = (target + _rn(g, b, h, w)).contiguous()
    tsmooth = kernels.median_blur5(target)
    scales = torch.tensor([1.0, 0.1], device=DEV)

    def run():
        sums = kernels.edge_loss_sums(pred, target, tsmooth, 48.0)
        return None, {"sums": sums, "grad": kernels.edge_loss_grad(pred, target, tsmooth, 48.0, sums, scales)}
    return run


@case("loss/photometric", "kernels.photometric_sums", "kernels.photometric_grad")
def _():
    g = _gen(33)
    b, h, w = 3, 41, 67
    left, right = torch.rand((b, 3, h, w), generator=g).to(DEV), torch.rand((b, 3, h, w), generator=g).to(DEV)
    disp = (_rn(g, b, h, w).abs() * 5).contiguous()
    excl = (torch.rand((b, h, w), generator=g) < 0.05).to(DEV)
    scales = torch.tensor([0.15, 0.85], device=DEV)

    def run():
        sums, warped, err = kernels.photometric_sums(left, right, disp, excl, want_warped=True, want_err=True)
        return None, {"sums": sums, "warped": warped, "err": err, "sums alone": kernels.photometric_sums(left, right, disp),
                      "grad": kernels.photometric_grad(left, right, disp, excl, sums=sums, scales=scales)}
    return run


@case("data/standardize_crop", "kernels.standardize_crop_u8")
def _():
    # (375, 1242) -> (384, 1248) scaled down: a padded crop (top and left), a cropping one, B = 3
    imgs = {(41, 67, 3): (_u8(34, 3, 41, 67, 3), _u8(35, 3, 41, 67, 3)),
            (41, 67, 4): (_u8(36, 41, 67, 4), _u8(37, 41, 67, 4))}

    def run():
        out = {}
        for key, (l, r) in imgs.items():
            for ch, cw in ((48, 72), (48, 70), (30, 40)):
                out[f"{key} -> {(ch, cw)} l"], out[f"{key} -> {(ch, cw)} r"] = kernels.standardize_crop_u8(l, r, ch, cw)
        return None, out
    return run


@case("data/train_transform", "kernels.train_transform_u8")
def _():
    from leastereo_amd import data
    import random
    g = _gen(38)
    b, h, w, ch, cw = 3, 41, 67, 32, 48
    l, r = _u8(38, b, h, w, 3), _u8(39, b, h, w, 3)
    dl, dr = (_rn(g, b, h, w).abs() * 20).contiguous(), (_rn(g, b, h, w).abs() * 20).contiguous()
    rng = random.Random(5)
    rows = [data.sample_train_params(h, w, ch, cw, True, False, 0, rng=rng),
            data.sample_train_params(h, w, ch, cw, False, True, 0, rng=rng),
            data.sample_train_params(h, w, ch, cw, True, False, 3, rng=rng)]
    params = torch.tensor(rows, dtype=torch.int32, device=DEV)
    pad = torch.tensor([data.center_params(h, w, 48, 72)] * b, dtype=torch.int32, device=DEV)

    def run():
        out = {}
        for tag, p, (th, tw) in (("crop", params, (ch, cw)), ("pad", pad, (48, 72))):
            for name, t in zip(("l", "r", "target", "n_valid"), kernels.train_transform_u8(l, r, dl, dr, p, th, tw, 48.0)):
                out[f"{tag} {name}"] = t
        out["no right n_valid"] = kernels.train_transform_u8(l, r, dl, None, params, ch, cw, 48.0)[3]
        return None, out
    return run


@case("data/tiles_and_blend", "kernels.standardize_tiles_u8", "kernels.blend_tiles")
def _():
    from leastereo_amd import scene
    th, tw, md, ctx, ramp = 96, 192, 48, 8, 8  # the small case of test_gpu_scene.py
    l, r = _u8(41, 150, 300, 3), _u8(42, 150, 300, 3)
    plan = scene.plan_tiles(150, 300, th, tw, md, context=ctx, ramp=ramp)
    origins = torch.tensor(plan.origins.tolist() + [[-5, -7], [150, 0], [140, 280]], dtype=torch.int32, device=DEV)
    g = _gen(43)
    tiles = _rn(g, len(plan), th, tw)
    holes = scene.TilePlan(150, 300, th, tw, md, ctx, ramp, [0, 54], [0])  # the right 116 columns have no tile
    tiles2 = _rn(g, 2, th, tw)

    def run():
        out = {}
        out["tiles l"], out["tiles r"] = kernels.standardize_tiles_u8(l, r, origins, th, tw)
        out["tiles l odd"], _ = kernels.standardize_tiles_u8(l, r, origins, th - 1, tw - 3)
        for view in ("left", "right"):
            out["blend " + view] = kernels.blend_tiles(tiles, plan, view)
        out["blend checked"] = kernels.blend_tiles(tiles, plan, "left", check=True)  # allocates its own count
        count = torch.empty(1, device=DEV, dtype=torch.int32)
        out["blend holes"] = kernels.blend_tiles(tiles2, holes, "left", count=count)
        out["hole count"] = count
        return None, out
    return run


@case("data/metrics", "kernels.disparity_metrics")
def _():
    g = _gen(44)
    gt = (_rn(g, 3, 41, 67).abs() * 20).contiguous()
    gt[:, ::5, ::3] = 0.0
    pred = (gt + _rn(g, 3, 41, 67, s=2.0)).contiguous()

    def run():
        counts, mask = kernels.disparity_metrics(pred, gt, 48.0, correct_mask=True)
        counts2, _ = kernels.disparity_metrics(pred[0], gt[0], 48.0, round_pred=True, z_shift=1)
        return None, {"counts": counts, "mask": mask, "counts rounded": counts2}
    return run


# ------------------------------------------------------------------------------------ training
def _convbr_case(shape, k, kind, training, relu):
    def factory():
        from leastereo_amd.training import _ConvBRFn
        b, cin, cout = shape[:3]
        sp = tuple(shape[3:])
        g = _gen(7 + cin * 31 + cout)
        stride = 3 if kind == "s3" else 1
        so = sp if kind == "3d" else (1,) + tuple((n - 1) // stride + 1 for n in sp)
        si = sp if kind == "3d" else (1,) + sp
        x = _rn(g, b, cin, *si)
        wt = (_w3(g, cout, cin, k) if kind == "3d" else _w2(g, cout, cin))
        gam, bet = 1 + 0.2 * _rn(g, cout), 0.1 * _rn(g, cout)
        rm0, rv0 = 0.1 * _rn(g, cout), 1 + torch.rand(cout, generator=g).to(DEV)
        dy = _rn(g, b, cout, *so)

        def run():
            xd, wd = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
            gd, bd = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
            rm, rv = rm0.clone(), rv0.clone()
            y = _ConvBRFn.apply(xd, wd, gd, bd, rm, rv, training, 0.1, 1e-5, True, relu, kind)
            y.backward(dy)
            return None, {"y": y, "dx": xd.grad, "dw": wd.grad, "dgamma": gd.grad, "dbeta": bd.grad,
                          "running_mean": rm, "running_var": rv}
        return run
    return factory


_TRAIN_COVERS = ("training.convbr3d", "training.conv3d_wgrad", "training.flip_weights", "training.conv2d_wgrad",
                 "training.conv2d_s3_backward")
for _shape, _k, _kind, _tr, _relu in [((2, 3, 5, 1, 1, 1), 3, "3d", True, True),
                                      ((1, 4, 80, 2, 3, 7), 3, "3d", True, False),
                                      ((2, 8, 8, 6, 10, 70), 3, "3d", True, True),
                                      ((1, 3, 16, 20, 33), 3, "2d", True, True),
                                      ((1, 5, 40, 7, 8), 3, "s3", False, True)]:
    CASES["train/convbr/" + "x".join(map(str, _shape)) + "-" + _kind] = (
        _TRAIN_COVERS, _convbr_case(_shape, _k, _kind, _tr, _relu))


@case("train/interpolate_disparity_costvolume", "training.resample3d_backward", "training.disparity_regression",
      "training.build_cost_volume")
def _():
    from leastereo_amd import training
    g = _gen(45)
    xs = [(_rn(g, 2, 3, 9, 7, 13), (5, 4, 7), True), (_rn(g, 1, 2, 1, 2, 3), (4, 1, 6), False)]
    dys = [_rn(g, *x.shape[:2], *size) for x, size, _ in xs]
    cost, dout = _cost(g, 1, 6, 3, 4), _rn(g, 1, 9, 12)
    fl, fr, dcost = _rn(g, 1, 3, 2, 5), _rn(g, 1, 3, 2, 5), _rn(g, 1, 6, 10, 2, 5)

    def run():
        out = {}
        for (x, size, ac), dy in zip(xs, dys):
            xd = x.clone().requires_grad_(True)
            y = training.interpolate3d(xd, size, ac)
            y.backward(dy)
            out[f"interp {size} y"], out[f"interp {size} dx"] = y, xd.grad
        c = cost.clone().requires_grad_(True)
        d = training.disparity_regression(c, 17)
        d.backward(dout)
        out["disp"], out["dcost"] = d, c.grad
        l, r = fl.clone().requires_grad_(True), fr.clone().requires_grad_(True)
        v = training.build_cost_volume(l, r, 30)
        v.backward(dcost)
        out["volume"], out["dl"], out["dr"] = v, l.grad, r.grad
        return None, out
    return run


# ------------------------------------------------------------------------------------ the comparison
def _compare(cid, byte, got, want):
    under = "a second plain run" if byte is None else f"the run under 0x{byte:02X}"
    assert sorted(got) == sorted(want), (cid, sorted(set(got) ^ set(want)))
    for name, w in want.items():
        gt = got[name]
        if name.startswith("pattern/"):
            if byte is not None:
                held = gt.contiguous().view(torch.uint8)
                bad = int((held != byte).sum())
                assert bad == 0, f"{cid}, {under}: {bad} bytes of {name} beside the slice were written"
            continue
        assert (gt is None) == (w is None), (cid, name)
        if w is None:
            continue
        assert gt.shape == w.shape and gt.dtype == w.dtype, (cid, name, gt.shape, w.shape, gt.dtype, w.dtype)
        a, b = dm.bits(gt), dm.bits(w)
        if not torch.equal(a, b):
            diff = (a != b).nonzero()
            raise AssertionError(
                f"{cid}: {name} {tuple(w.shape)} {w.dtype}: {under} differs from the plain run in "
                f"{diff.shape[0]} of {a.numel()} elements, first at {diff[0].tolist()}: "
                f"{gt[tuple(diff[0])].item()!r} for {w[tuple(diff[0])].item()!r}")


@pytest.mark.parametrize("cid", sorted(CASES))
def test_same_bits_from_poisoned_buffers(cid):
    run = CASES[cid][1]()
    torch.cuda.synchronize()
    route, want = run()
    torch.cuda.synchronize()
    again = run()[1]  # two plain runs first: a difference here is no matter of memory
    torch.cuda.synchronize()
    _compare(cid, None, again, want)
    failures = []  # every pattern runs, so that a report names each one that differs
    for byte in dm.PATTERNS:
        with dm.dirty(byte, DEV) as mem:
            r, got = run()
            torch.cuda.synchronize()
            mem.check()
            assert mem.allocations, f"{cid}: nothing was allocated through the patched names"
        assert r == route, (cid, byte, r, route)
        try:
            _compare(cid, byte, got, want)
            if hasattr(run, "judge"):
                run.judge(got)
        except AssertionError as e:
            failures.append(f"0x{byte:02X}: {e}")
    assert not failures, "\n".join(failures)


def test_a_write_past_a_guarded_tensor_is_seen():
    """The guard path, without touching a kernel: one element past a guarded tensor."""
    with dm.dirty(dm.NAN, DEV) as mem:
        t = torch.empty((3, 5), device=DEV)
        torch.empty(7, device=DEV, dtype=torch.int32)
        mem.check()
        t.as_strided((1,), (1,), t.storage_offset() + t.numel()).fill_(1.0)  # lands in the helper's own guard
        with pytest.raises(AssertionError, match="after allocation #0"):
            mem.check()
    with dm.dirty(dm.NAN, DEV) as mem:
        t = torch.empty((3, 5), device=DEV, dtype=torch.uint8)
        t.as_strided((1,), (1,), t.storage_offset() - 1).fill_(1)
        with pytest.raises(AssertionError, match="before allocation #0"):
            mem.check()


# ------------------------------------------------------------------------------------ the whole model
H, W, MD = 96, 192, 48


def _model(precision):
    from leastereo_amd.config import LEAStereoArgs, default_arch_args
    from leastereo_amd.model import LEAStereo
    from tests.golden_util import state_dict
    m = LEAStereo(default_arch_args(LEAStereoArgs(maxdisp=MD)), DEV, precision=precision)
    m.load_state_dict(state_dict(), strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _pair(seed):
    from tests.golden_util import normal
    return normal(seed, (1, 3, H, W)).to(DEV), normal(seed + 1, (1, 3, H, W)).to(DEV)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_eval_forward_on_recycled_memory(precision):
    """Input A under 0xFF, then input B under 0x55 on the same model (whatever it keeps between
    forwards now holds A's values or the first pattern), each against a plain forward of the same
    input on a fresh model."""
    want = {}
    for seed in (101, 201):
        with torch.no_grad():
            want[seed] = _model(precision).eval()(*_pair(seed))
    torch.cuda.synchronize()
    m = _model(precision).eval()
    for seed, byte in ((101, dm.NAN), (201, dm.BIG)):
        with dm.dirty(byte, DEV) as mem, torch.no_grad():
            got = m(*_pair(seed))
            torch.cuda.synchronize()
            mem.check()
            assert len(mem.allocations) > 50
        _compare(f"forward {precision} input {seed}", byte, {"disp": got}, {"disp": want[seed]})
        assert bool(torch.isfinite(got).all())


def _train_step(m):
    from tests.golden_util import normal
    left, right = (t.clone().requires_grad_(True) for t in _pair(311))
    target = normal(313, (1, H, W)).to(DEV) * 4 + 20
    disp = m(left, right)
    mask = (target < MD) & (target > 0.001)
    loss = torch.nn.functional.smooth_l1_loss(disp[mask], target[mask], reduction="mean")
    loss.backward()
    out = {"loss": loss.detach(), "disp": disp.detach(), "d_left": left.grad, "d_right": right.grad}
    out.update({"grad/" + n: p.grad for n, p in m.named_parameters()})
    out.update({"buffer/" + n: b for n, b in m.named_buffers()})
    return out


def test_train_step_on_recycled_memory():
    """One train step (test_gpu_training.py::test_whole_model_train_step_vs_reference_golden's):
    loss, disparity, every parameter gradient and the running statistics."""
    want = _train_step(_model("f32").train())
    torch.cuda.synchronize()
    for byte in (dm.NAN, dm.BIG):
        m = _model("f32").train()
        with dm.dirty(byte, DEV) as mem:
            got = _train_step(m)
            torch.cuda.synchronize()
            mem.check()
        _compare("train step", byte, got, want)


def test_scene_of_two_tiles_on_recycled_memory():
    from leastereo_amd import scene
    from tests.golden_util import golden
    g = golden("c1_sceneflow")
    left, right = (torch.from_numpy(np.ascontiguousarray(g[k][:H, :300])).to(DEV) for k in ("left_u8", "right_u8"))
    kw = dict(tile_batch=1, context=8, ramp=8, confidence=True, radius=3, lr_threshold=1.0, graph=False)
    runner = scene.SceneRunner(_model("f32").eval(), H, W, **kw)
    assert len(runner.plan(H, 300)) == 2
    want = runner(left, right)
    torch.cuda.synchronize()
    for byte in (dm.NAN, dm.BIG):
        fresh = scene.SceneRunner(_model("f32").eval(), H, W, **kw)
        with dm.dirty(byte, DEV) as mem:
            got = fresh(left, right)
            torch.cuda.synchronize()
            mem.check()
        _compare("scene", byte, dict(got._asdict()), dict(want._asdict()))
