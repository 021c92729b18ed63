"""The judges of the feature net's 2D kernels and of the factored matching stem0 (CPU only:
torch / numpy, no GPU import; nothing here is taken from a kernel).  The methods are those of
tests/bf16_judge.py (exact integer recipes, half a bf16 ulp + 4 e32) and tests/f32_judge.py
(a float32 restatement's own error in units of S); this module only states the operations.

2D 3x3 convs (csrc/conv2d_small.hip, the 2D tiles of csrc/conv3d.hip, csrc/conv2d_s3.hip):
float64 torch is the reference, and the float32 model is f32_judge.direct_f32 on the conv
embedded as a D = 1 volume, the 3 x 3 weight on the kd = 1 slab between two slabs of zeros --
exactly equivalent, a zero product does not move a float32 accumulator.  The stride-3 conv
(pad 1) reads rows 3 ho - 1 .. 3 ho + 1: the stride-1 conv at every third row and column.

Fused stems (csrc/feature_stem.hip): relu(BN1(conv_s3(relu(BN0(conv(x)))))) with stem1's zero
padding applied to stem0's *activation* -- the ring reads 0, not relu(shift0).

Factored stem0 (csrc/cv_stem.hip): ``split_weights`` / ``combine`` restate
lea_cv_stem_split_weights / lea_cv_stem_combine; the f32 judge is the conv over the
materialised cost volume (bf16_judge.costvolume_judge), the c8 judge models the one rounding
the path adds by design, the maps' store as bf16: epilogue(combine(rn_bf16(maps))), with e32 the
float32 evaluation of that expression on the same rounded maps (``stem0_c8_e32``).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import bf16_judge as B
from tests import f32_judge as F32

MARGIN = F32.MARGIN
CAP = F32.CAP


# ------------------------------------------------------------------------------ 2D convs
def conv2d_raw(x, w, stride=1, dtype=torch.float64):
    """The plain 3 x 3 conv, zero padding 1, stride 1 or 3: x [B, C, H, W], w [O, C, 3, 3]."""
    return F.conv2d(x.to(dtype), w.to(dtype), None, stride, 1)


def embed3d(x, w):
    """x [B, C, H, W], w [O, C, 3, 3] (tensors or arrays) -> float32 arrays x [B, C, 1, H, W],
    w [O, C, 3, 3, 3] with w on the kd = 1 slab."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    w3 = np.zeros(w.shape[:2] + (3, 3, 3), np.float32)
    w3[:, :, 1] = w
    return x[:, :, None], w3


def conv2d_f32_model(x, w, stride=1, dtype=torch.float32):
    """f32_judge.direct_f32 on the embedded conv, [B, O, Ho, Wo] float32 array."""
    x3, w3 = embed3d(x, w)
    return F32.direct_f32(x3, w3, 3, dtype=dtype)[:, :, 0, ::stride, ::stride]


def scale2d(x, w, stride=1):
    """S[b, co] = max over the outputs of conv(|x|, |w|), float64 (f32_judge.scale in 2D)."""
    return conv2d_raw(torch.as_tensor(x).abs(), torch.as_tensor(w).abs(), stride).amax(dim=(2, 3)).numpy()


def error2d(y, ref, s):
    """E = max |y - ref| / S[b, co]."""
    d = np.abs(np.asarray(y, np.float64) - np.asarray(ref, np.float64))
    return float((d / s.reshape(s.shape + (1,) * (d.ndim - 2))).max())


def normal_conv2d(seed, cin, cout, hw, batch=2):
    """float32 N(0, 1) activations and N(0, 1) / sqrt(9 cin) weights (not rounded to bf16: the
    f32 paths' inputs), from numpy's PCG64 as f32_judge.inputs."""
    rng = np.random.default_rng([seed, cin, cout, hw[0], hw[1]])
    x = rng.standard_normal((batch, cin) + tuple(hw), dtype=np.float32)
    w = rng.standard_normal((cout, cin, 3, 3), dtype=np.float32) / np.float32(np.sqrt(9 * cin))
    return torch.from_numpy(x), torch.from_numpy(w)


class Judged2d:
    """One pure conv on normal_conv2d's inputs: ref64, S and the float32 model's E."""

    def __init__(self, seed, cin, cout, hw, batch=2, stride=1):
        self.x, self.w = normal_conv2d(seed, cin, cout, hw, batch)
        self.ref = conv2d_raw(self.x, self.w, stride).numpy()
        self.s = scale2d(self.x, self.w, stride)
        self.e_model = error2d(conv2d_f32_model(self.x, self.w, stride), self.ref, self.s)
        self.bar = MARGIN * self.e_model

    def error(self, y):
        return error2d(y, self.ref, self.s)


@functools.lru_cache(maxsize=8)
def judged2d(seed, cin, cout, hw, batch=2, stride=1):
    return Judged2d(seed, cin, cout, hw, batch, stride)


def bn_draw(g, cout, scales, lo, hi):
    """Per-channel scale drawn from ``scales`` and an integer shift in [lo, hi]."""
    scale = torch.tensor(scales)[torch.randint(0, len(scales), (cout,), generator=g)]
    return scale, torch.randint(lo, hi + 1, (cout,), generator=g).float()


def integer_s3_case(seed, cin, cout, hw, batch=2):
    """bf16_judge.integer_case for the stride-3 conv (no residual there): ternary inputs, every
    activation exact in bf16 (asserted on the reference), so in float32 as well."""
    g = torch.Generator().manual_seed(seed)
    x = B._ternary(g, (batch, cin) + tuple(hw), 0.5)
    w = B._ternary(g, (cout, cin, 3, 3), 0.25)
    scale, shift = bn_draw(g, cout, [0.5, 1.0, 2.0], -4, 4)
    B.assert_integer_exact(conv2d_raw(x, w, 3), scale, shift, torch.zeros(1))
    return dict(x=x, w=w, scale=scale, shift=shift)


def s3_judge(x, w, scale, shift, relu, dtype=torch.float64):
    return B.epilogue(conv2d_raw(x, w, 3, dtype), scale, shift, relu)


# ------------------------------------------------------------------------------ fused stems
STEM_CIN, STEM_C0, STEM_C1 = 3, 16, 32   # the one instantiation (feature_stem.hip:169)


def stem0_act(x, w0, scale0, shift0, dtype=torch.float64):
    return B.epilogue(conv2d_raw(x, w0, 1, dtype), scale0, shift0, True)


def stem_judge(x, w0, scale0, shift0, w1, scale1, shift1, dtype=torch.float64):
    """relu(BN1(conv_s3(relu(BN0(conv(x)))))), unrounded, in ``dtype``."""
    return B.epilogue(conv2d_raw(stem0_act(x, w0, scale0, shift0, dtype), w1, 3, dtype), scale1, shift1, True)


def stem_args(c):
    return c["x"], c["w0"], c["scale0"], c["shift0"], c["w1"], c["scale1"], c["shift1"]


def integer_stem_case(seed, hw, batch=2):
    """Ternary image and weights (image and w0 non-zero with probability 0.5, w1 0.25), scale0 in
    {0.5, 1, 2}, shift0 an integer in [-2, 2] and POSITIVE on several channels (so that
    relu(shift0) in stem1's padding ring would differ from the 0 that belongs there), scale1 in
    {0.5, 1}, shift1 an integer in [-4, 4].  Every sum is a multiple of 1/4 far below 2^24 * 1/4,
    exact in float32 in any order, with or without FMA contraction; asserts ON THE REFERENCE ALONE
    that the final activation is unchanged by rn_bf16."""
    g = torch.Generator().manual_seed(seed)
    x = B._ternary(g, (batch, STEM_CIN) + tuple(hw), 0.5)
    w0 = B._ternary(g, (STEM_C0, STEM_CIN, 3, 3), 0.5)
    w1 = B._ternary(g, (STEM_C1, STEM_C0, 3, 3), 0.25)
    scale0, shift0 = bn_draw(g, STEM_C0, [0.5, 1.0, 2.0], -2, 2)
    scale1, shift1 = bn_draw(g, STEM_C1, [0.5, 1.0], -4, 4)
    c = dict(x=x, w0=w0, scale0=scale0, shift0=shift0, w1=w1, scale1=scale1, shift1=shift1)
    assert int((shift0 > 0).sum()) >= 3, "shift0 must be positive on several stem0 channels"
    a = stem0_act(x, w0, scale0, shift0)
    raw1 = conv2d_raw(a, w1, 3)
    assert torch.equal(a * 2, (a * 2).round()) and torch.equal(raw1 * 2, (raw1 * 2).round())
    assert float(raw1.abs().max()) * 4 < 2 ** 24
    B.assert_bf16_exact(stem_judge(*stem_args(c)), "stem activation")
    return c


def normal_stem_case(seed, hw, batch=2):
    """The recipe of test_fused_feature_stems_vs_torch: a N(0, 1) image, weights / sqrt(fan in),
    scales in 0.5-1.5, shifts 0.1 N, all float32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((batch, STEM_CIN) + tuple(hw), generator=g)
    w0 = torch.randn(STEM_C0, STEM_CIN, 3, 3, generator=g) / float(9 * STEM_CIN) ** 0.5
    w1 = torch.randn(STEM_C1, STEM_C0, 3, 3, generator=g) / float(9 * STEM_C0) ** 0.5
    return dict(x=x, w0=w0, scale0=torch.rand(STEM_C0, generator=g) + 0.5,
                shift0=torch.randn(STEM_C0, generator=g) * 0.1, w1=w1,
                scale1=torch.rand(STEM_C1, generator=g) + 0.5, shift1=torch.randn(STEM_C1, generator=g) * 0.1)


def _bn_relu_f32(c, scale, shift):
    """float32 numpy epilogue as f32_judge.chain_f32: product, sum and max each rounded."""
    bc = (None, slice(None), None, None)
    y = np.maximum(c * np.asarray(scale, np.float32)[bc] + np.asarray(shift, np.float32)[bc], np.float32(0))
    assert y.dtype == np.float32
    return y


def stem_chain_f32(x, w0, scale0, shift0, w1, scale1, shift1):
    """The two-layer chain in float32 with every product and sum rounded (f32_judge.direct_f32
    for the convs, numpy for the epilogues)."""
    a = _bn_relu_f32(conv2d_f32_model(x, w0), scale0, shift0)
    return _bn_relu_f32(conv2d_f32_model(a, w1, 3), scale1, shift1)


def rel_error(y, ref):
    """max |y - ref| / max |ref| (f32_judge.chain_error's measure)."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------------------ factored stem0
def split_weights(w):
    """lea_cv_stem_split_weights restated: [cout, 2C, 3, 3, 3] -> wl [9 cout, C, 3, 3],
    wr [6 cout, C, 3, 3]."""
    cout, c2 = w.shape[:2]
    c = c2 // 2
    wl = torch.zeros(9 * cout, c, 3, 3, dtype=w.dtype)
    wr = torch.zeros(6 * cout, c, 3, 3, dtype=w.dtype)
    for kd in range(3):
        for t in range(3):
            blk = w[:, :c, kd].clone()
            blk[..., :t] = 0
            wl[(3 * kd + t) * cout:(3 * kd + t + 1) * cout] = blk
        wr[kd * cout:(kd + 1) * cout] = w[:, c:, kd]
        wr[(3 + kd) * cout:(4 + kd) * cout, :, :, 1] = w[:, c:, kd, :, 2]
    return wl, wr


def combine(lm, rm, cout, d3, edge_shift=0, z_minus_1=True):
    """lea_cv_stem_combine's sum (pre-BN), restated with explicit loops over planes.
    ``edge_shift`` / ``z_minus_1`` plant defects (the last-column correction taken that many
    columns off, the z = -1 term dropped) for tests/test_judges_feature_cpu.py."""
    b, _, h, wd = lm.shape
    lk = lm.view(b, 3, 3, cout, h, wd)
    bk = rm[:, :3 * cout].view(b, 3, cout, h, wd)
    k2 = rm[:, 3 * cout:].view(b, 3, cout, h, wd)
    out = torch.zeros(b, cout, d3, h, wd, dtype=lm.dtype)
    cols = torch.arange(wd)
    for d in range(d3):
        u = cols - d
        for kd in range(3):
            if not 0 <= d + kd - 1 < d3:
                continue
            t = (kd - u).clamp(min=0)
            left = torch.zeros(b, cout, h, wd, dtype=lm.dtype)
            for tv in range(3):
                sel = t == tv
                left[..., sel] = lk[:, kd, tv][..., sel]
            z = u - kd + 1
            right = torch.zeros_like(left)
            ok = (z >= 0) & (z < wd)
            right[..., ok] = bk[:, kd][..., z[ok]]
            if z_minus_1:
                right[..., z == -1] = k2[:, kd][..., 0:1].expand_as(right[..., z == -1])
            x = u[-1] - kd + 2 + edge_shift  # last column: taps past the volume's right edge
            if 0 <= x < wd:
                right[..., -1] -= k2[:, kd][..., x]
            out[:, :, d] += left + right
    return out


def stem0_maps(fl, fr, w, dtype=torch.float64):
    """The 2D maps the factored kernel combines: (lm [B, 9 cout, H, W], rm [B, 6 cout, H, W])."""
    wl, wr = split_weights(w.to(dtype))
    return F.conv2d(fl.to(dtype), wl, None, 1, 1), F.conv2d(fr.to(dtype), wr, None, 1, 1)


def stem0_from_maps(lm, rm, cout, d3, scale, shift, relu=True, **defect):
    """epilogue(combine(maps)) in the maps' dtype."""
    return B.epilogue(combine(lm, rm, cout, d3, **defect), scale, shift, relu)


def stem0_c8_judge(fl, fr, maxdisp, w, scale, shift, relu=True, dtype=torch.float64):
    """epilogue(combine(rn_bf16(maps))): the maps are stored as bf16 before the f32 sum
    (tests/test_gpu_cv_stem.py:7-8), the one rounding the c8 path adds to the volume conv."""
    lm, rm = stem0_maps(fl, fr, w, dtype)
    return stem0_from_maps(B.rn_bf16(lm).to(dtype), B.rn_bf16(rm).to(dtype), w.shape[0], maxdisp // 3,
                           scale, shift, relu)


def stem0_c8_e32(lm_bf, rm_bf, cout, d3, scale, shift, relu=True):
    """The c8 judge's e32: epilogue(combine(.)) in float32 against float64 on the SAME bf16 maps.
    The maps' rounding points are taken from the float64 maps and not re-derived in float32, for
    the reason bf16_judge.pair_wants gives: a float32 restatement of the map convs rounds some map
    the other way at a near tie and would report that whole bf16 ulp of a map -- 1e-5 .. 2e-3 on
    the cases here, as many as a few per case -- as "float32 error"."""
    return B.e32_of(stem0_from_maps(lm_bf.float(), rm_bf.float(), cout, d3, scale, shift, relu),
                    stem0_from_maps(lm_bf.double(), rm_bf.double(), cout, d3, scale, shift, relu))


def normal_costvolume_f32(seed, c, cout, maxdisp, hw, batch=2):
    """bf16_judge.normal_costvolume_case without the rounding to bf16 (the f32 path's inputs)."""
    g = torch.Generator().manual_seed(seed)
    fl = torch.randn((batch, c) + tuple(hw), generator=g)
    fr = torch.randn((batch, c) + tuple(hw), generator=g)
    w = torch.randn(cout, 2 * c, 3, 3, 3, generator=g) / float(2 * c * 27) ** 0.5
    return dict(fl=fl, fr=fr, w=w, scale=torch.rand(cout, generator=g) + 0.5,
                shift=torch.randn(cout, generator=g) * 0.1)


def stem0_f32_models(fl, fr, maxdisp, w):
    """The pure volume conv (no epilogue) on float32 inputs: (ref64, S, E of the float32 combine
    of float32 maps, E of direct_f32 on the materialised volume); the maps by conv2d_f32_model,
    the combine's sums in float32 torch."""
    cout, d3 = w.shape[0], maxdisp // 3
    vol = B.build_cost_volume(fl, fr, maxdisp, torch.float32).numpy()
    wn = w.numpy()
    ref, s = F32.ref64(vol, wn, 3), F32.scale(vol, wn)
    wl, wr = split_weights(w)
    lm = torch.from_numpy(np.ascontiguousarray(conv2d_f32_model(fl, wl)))
    rm = torch.from_numpy(np.ascontiguousarray(conv2d_f32_model(fr, wr)))
    e_comb = F32.error(combine(lm, rm, cout, d3).numpy(), ref, s)[0]
    e_direct = F32.error(F32.direct_f32(vol, wn, 3), ref, s)[0]
    return ref, s, e_comb, e_direct


def integer_stem0_case(seed, c, cout, maxdisp, hw, batch=2):
    """bf16_judge.integer_costvolume_case, asserting besides (on the reference alone) that both
    map stacks are exact in bf16 and that combine(maps) equals the volume conv bit for bit in
    float64 -- so the f32 and the c8 path must both return the materialised conv exactly."""
    f = B.integer_costvolume_case(seed, c, cout, maxdisp, hw, batch)
    lm, rm = stem0_maps(f["fl"], f["fr"], f["w"])
    B.assert_bf16_exact(lm, "left maps")
    B.assert_bf16_exact(rm, "right maps")
    raw = B.conv_raw(B.build_cost_volume(f["fl"], f["fr"], maxdisp), f["w"], 3)
    assert torch.equal(combine(lm, rm, cout, maxdisp // 3), raw), "combine(maps) != volume conv"
    return f


# ---- the cases of tests/test_gpu_feature_exact.py (their preconditions: test_judges_feature_cpu.py) ----
HW_RAGGED = (9, 35)   # a second 32-column tile 3 wide, a ragged row tile for TH = 8, 4 and 2
# conv2d_small_kernel<CIN, NG>: CIN = cin rounded up to 4, NG = 1 / 2 / 4 for cout <= 8 / 16 / 32;
# all twelve, cin in {3, 4, 5, 8, 9, 12, 13, 16} over cout in {5, 8, 12, 16, 20, 24, 32}
SMALL = [(3, 5), (4, 16), (3, 32), (5, 8), (8, 12), (5, 20), (9, 5), (12, 16), (9, 24), (13, 8), (16, 12),
         (16, 32), (4, 20), (8, 24)]
SMALL_SHAPES = [(HW_RAGGED, 2), ((1, 1), 2)]
# lea_conv2d_bnrelu_pair: (cin, c1, cout)
PAIR = [(8, 8, 16), (16, 16, 32), (5, 8, 32), (12, 16, 24)]
# the 2D DMA / MFMA engine: (cin, cout, hw, batch) -> (mt, nt); nt = 2 needs 512 workgroups
DMA2D = {
    (5, 16, (9, 35), 1): (1, 1), (32, 32, (9, 36), 1): (2, 1), (64, 48, (9, 35), 1): (3, 1),
    (32, 64, (9, 36), 1): (4, 1), (64, 96, (9, 35), 1): (3, 1), (32, 192, (9, 36), 1): (4, 1),
    (32, 16, (123, 250), 2): (1, 2), (5, 32, (123, 250), 2): (2, 2), (5, 48, (123, 250), 2): (3, 2),
    (5, 64, (123, 250), 2): (4, 2),
}
# Hi mod 3 and Wi mod 3 each 0, 1, 2; Wo = 66 / 67 crosses the fused kernel's 64-column seam,
# Ho = 8 its 4-row seam; on the last every output touches padding
S3_SHAPES = [(22, 198), (23, 200), (24, 199), (4, 3)]
S3 = [(5, 20), (16, 32)]
STEM_SHAPES = [(22, 198), (23, 200), (24, 199), (5, 7)]
# lea_cv_stem_combine: (C, cout, maxdisp, hw, batch).  f32 walks min(D3, 544) planes per workgroup
# and c8 min(D3, 224) (cv_stem.hip:53-55 and the dchunk of lea_cv_stem_combine: 80 KB of LDS for
# ob (2 dchunk + 191) floats, ob = 16 / 32), so D3 = 545 / 225 are the smallest that split.
CV_F32 = [(32, 32, 48, (6, 72), 2), (16, 16, 27, (5, 68), 2), (8, 48, 24, (4, 20), 2), (32, 32, 24, (4, 132), 2),
          (4, 16, 27, (5, 8), 2), (8, 24, 12, (3, 64), 2), (4, 8, 3 * 545, (2, 8), 1)]
CV_C8 = [(16, 16, 27, (5, 19), 2), (16, 40, 12, (3, 19), 2), (32, 32, 48, (6, 70), 2),
         (16, 16, 3 * 225, (2, 24), 1)]
KINDS = ("int", "normal")


def seed_of(*key):
    """A case's seed from its key (a name, ints and tuples of ints)."""
    flat = [v for k in key for v in (k if isinstance(k, tuple) else (k,))]
    return sum((i + 1) * (len(v) if isinstance(v, str) else int(v)) for i, v in enumerate(flat)) % 100003


# Seeds whose integer recipe misses its own precondition (a half-integer above 128, say) are
# replaced here, by hand and from the reference alone: key -> seed.
SEEDS = {("stem", (5, 7), 2): 0}   # the derived seed draws fewer than three positive shift0


def _seed(*key):
    return SEEDS.get(key, seed_of(*key))


@functools.lru_cache(maxsize=4)
def conv2d_int(cin, cout, hw, batch):
    return B.integer_case(_seed("conv2d", cin, cout, hw, batch), cin, cout, 3, hw, batch)


def conv2d_normal(cin, cout, hw, batch, stride=1):
    return judged2d(_seed("conv2d", cin, cout, hw, batch), cin, cout, hw, batch, stride)


@functools.lru_cache(maxsize=4)
def s3_int(cin, cout, hw, batch=2):
    return integer_s3_case(_seed("s3", cin, cout, hw, batch), cin, cout, hw, batch)


@functools.lru_cache(maxsize=8)
def stem_case(kind, hw, batch=2):
    """The case with its float64 judge ("want"), the float32 torch judge's distance from it
    ("e32", the c8 output's) and, normal kind, the float32 chain restatement's error relative to
    max |want| ("e_chain", the f32 output's)."""
    c = dict((integer_stem_case if kind == "int" else normal_stem_case)(_seed("stem", hw, batch), hw, batch))
    c["want"] = stem_judge(*stem_args(c))
    c["e32"] = B.e32_of(stem_judge(*stem_args(c), dtype=torch.float32), c["want"])
    if kind == "normal":
        c["e_chain"] = rel_error(stem_chain_f32(*(t.numpy() for t in stem_args(c))), c["want"].numpy())
    return c


@functools.lru_cache(maxsize=4)
def cv_case(kind, prec, c, cout, maxdisp, hw, batch):
    """prec "f32" / "c8".  int: the exact materialised conv ("want", both precisions).  normal f32:
    float32 inputs, the pure conv's ref64 / S / model errors.  normal c8: bf16-rounded inputs, the
    c8 judge and its e32, and the float64 maps with their float32 distance (the 2D entry's bar)."""
    seed = _seed("cv", c, cout, maxdisp, hw, batch)
    if kind == "int":
        f = dict(integer_stem0_case(seed, c, cout, maxdisp, hw, batch))
        f["want"] = B.costvolume_judge(f["fl"], f["fr"], maxdisp, f["w"], f["scale"], f["shift"], True)
        return f
    if prec == "f32":
        f = dict(normal_costvolume_f32(seed, c, cout, maxdisp, hw, batch))
        f["ref"], f["s"], f["e_comb"], f["e_direct"] = stem0_f32_models(f["fl"], f["fr"], maxdisp, f["w"])
        f["bar"] = MARGIN * max(f["e_comb"], f["e_direct"])
        return f
    f = dict(B.normal_costvolume_case(seed, c, cout, maxdisp, hw, batch))
    args = (f["fl"], f["fr"], maxdisp, f["w"], f["scale"], f["shift"])
    f["want"] = stem0_c8_judge(*args)
    f["lm"], f["rm"] = stem0_maps(f["fl"], f["fr"], f["w"])
    f["e32"] = stem0_c8_e32(B.rn_bf16(f["lm"]), B.rn_bf16(f["rm"]), cout, maxdisp // 3, f["scale"], f["shift"])
    lm32, rm32 = stem0_maps(f["fl"], f["fr"], f["w"], torch.float32)
    f["e32_maps"] = max(B.e32_of(lm32, f["lm"]), B.e32_of(rm32, f["rm"]))
    return f
