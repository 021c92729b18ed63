"""The feature net's 2D kernels and the factored matching stem0 against the judges of
tests/feature_judge.py, on every dispatch path: the twelve conv2d_small_kernel<CIN, NG>
instantiations, lea_conv2d_bnrelu_pair, the eight (mt, nt) tiles of the 2D DMA / MFMA engine,
lea_conv2d_s3_bnrelu, lea_feature_stem_bnrelu (f32 and c8) and lea_cv_stem_combine (f32 and c8,
the maps built by lea_conv2d_bnrelu[_bf16] as the executor does).

Every case runs in two kinds.  "int": integer recipes on which every sum and every rounding point
is exact (asserted on the reference, tests/test_judges_feature_cpu.py), so the output must EQUAL
the float64 judge bit for bit -- a wrong tap, border, seam, channel block or edge correction
cannot hide.  "normal": N(0, 1) inputs; an f32 path runs as a pure conv and must meet
E(path) <= 4 x E(float32 model) in units of S (tests/f32_judge.py), the fused stems 4 x the float32
chain restatement's error relative to max |ref|, lea_cv_stem_combine 4 x max(E(float32 combine of
float32 maps), E(direct_f32 on the volume)); a c8 output must lie within half a bf16 ulp + 4 e32 of
the float64 value (bf16_judge.assert_half_ulp).

The c8 stem0 is judged through the maps the device stored.  Its judge is
epilogue(combine(rn_bf16(maps))), but where a float64 map value sits within the map conv's own
float32 error of a rounding tie the bf16 engine may store the neighbouring bf16 value, and both are
correct (bf16_judge.pair_wants has the same case): so the maps must lie within half an ulp + 4 e32 of
the float64 maps (the bf16 engine's 2D entry at couts 9 x cout and 6 x cout), and the output within
half an ulp + 4 e32 of epilogue(combine(those stored maps)) in float64, e32 that expression's
float32 distance (feature_judge.stem0_c8_e32).  "moved" in the c8 lines counts the outputs that this
changes against the float64 maps rounded on the CPU.

Outputs go into a channel slice between two sentinel slices (f32: 8 channels either side; c8: a
block either side), each launch's kernel is asserted through kernels.conv2d_kernel_name where a
name query exists, lea_conv2d_set_small is restored in a finally.  Each launch prints one JSON line
(pytest -s): int -- the differing elements; normal -- the figures, "share" of elements beyond the
bar and "used" = error / model error (f32) or (|got - fp64| - half ulp) / e32 (c8), which the
margin 4 has to cover.

Measured on an MI355X with the margin at 4: no differing element on the integer recipe, no
element beyond a bar on any path.  Worst "used" per path:

    path                                  int   normal   model / e32            worst used   at
    conv2d_small_kernel, all twelve       112     28     5.1e-08 .. 2.3e-07 S      1.25      8->24 (9, 35)
    lea_conv2d_bnrelu_pair                  8      4     1.5e-07 .. 1.9e-07 S      1.08      12->16+8
    2D DMA / MFMA engine, all eight        40     10     1.5e-07 .. 2.5e-07 S      1.13      64->96 (9, 35)
    lea_conv2d_s3_bnrelu                   16      8     7.8e-08 .. 2.7e-07 S      2.17      5->20 (4, 3)
    lea_feature_stem_bnrelu f32             4      4     2.3e-07 .. 5.6e-07        1.27      (22, 198)
    lea_feature_stem_bnrelu c8              4      4     7.7e-07 .. 1.5e-06        0.19      (22, 198)
    lea_cv_stem_combine f32                 7      7     1.3e-07 .. 3.2e-07 S      0.31      C8->24 md12 (3, 64)
    stem0's c8 maps (bf16 2D entry)         -      8     1.8e-07 .. 3.9e-07        0.14      C32->32 md48 (6, 70) left
    lea_cv_stem_combine c8                  4      4     1.8e-07 .. 4.4e-07        0.00      every case; 5 outputs
                                                                                             "moved" on md675
No kernel defect was found: the int kind passed on the first run.
"""
import json

import numpy as np
import pytest
import torch

from leastereo_amd import _lib, kernels
from tests import bf16_judge as B
from tests import feature_judge as J
from tests.test_gpu_bf16_exact import Sentinel, from_c8, to_c8

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.0
PAD = 8  # sentinel channels either side of an f32 output slice
KINDS = J.KINDS
# mode -> (relu, residual operand, accumulate)
MODES = {"plain": (True, False, False), "res": (True, True, False), "acc": (True, False, True),
         "norelu": (False, False, False)}


class SentinelF32:
    """An f32 output channel slice between two sentinel slices of PAD channels."""

    def __init__(self, b, cout, vol):
        self.big = torch.full((b, cout + 2 * PAD) + tuple(vol), SENTINEL, device=DEV)
        self.out = self.big[:, PAD:PAD + cout]

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.big[:, :PAD] == SENTINEL).all()), "the channels before the slice were written"
        assert bool((self.big[:, -PAD:] == SENTINEL).all()), "the channels after the slice were written"


def record(path, tag, kind, **st):
    """One JSON line per launch on stdout (pytest -s)."""
    print(json.dumps(dict(path=path, case=tag, kind=kind, **st)))


def judge_exact(path, tag, got, want):
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = int((got != want).sum())
    record(path, tag, "int", mismatches=bad, n=got.numel())
    assert torch.equal(got, want), f"{path} {tag}: {bad} of {got.numel()} elements differ from the exact result"


def judge_scaled(path, tag, y, ref, s, e_model, bar, **more):
    """An f32 path's pure conv: E = max |y - ref| / S within ``bar`` (MARGIN x its model)."""
    y = y.double().cpu().numpy()
    assert y.shape == ref.shape and np.isfinite(y).all(), (path, tag)
    d = np.abs(y - ref) / s.reshape(s.shape + (1,) * (y.ndim - 2))
    e = float(d.max())
    record(path, tag, "normal", E=e, model=e_model, bar=bar, share=float((d > bar).mean()), used=e / e_model,
           n=y.size, **more)
    assert e <= bar, f"{path} {tag}: E {e:.3e} > {bar:.3e} = {J.MARGIN} x model {e_model:.3e}"


def judge_c8(path, tag, got, want, e32, **more):
    try:
        st = B.assert_half_ulp(got, want, e32, tag=tag)
    except AssertionError:
        record(path, tag, "normal", **B.half_ulp_stats(got, want, e32), **more)
        raise
    record(path, tag, "normal", **st, **more)


def dev(t):
    return t.to(DEV).contiguous()


# ------------------------------------------------------------------ 2D 3x3 / s1 entry, f32
def small_name(cin, cout):
    return f"conv2d_small_kernel<{(cin + 3) // 4 * 4}, {1 if cout <= 8 else 2 if cout <= 16 else 4}>"


def dma2d_name(mt, nt):
    return f"conv3d_dma_kernel<{mt}, {nt}, 16, 1, 1, false>"


def run_conv2d(x, packed, cout, scale, shift, r, mode):
    """One launch of lea_conv2d_bnrelu into a sentinel-guarded slice; x, r [B, C, 1, H, W]."""
    relu, res, acc = MODES[mode]
    s = SentinelF32(x.shape[0], cout, (1,) + tuple(x.shape[3:]))
    if acc:
        s.out.copy_(r)
    kernels.conv2d_bnrelu(x, packed, cout, scale, shift, relu=relu, out=s.out, accumulate=acc,
                          residual=r if res else None)
    s.check()
    return s.out[:, :, 0]


def conv2d_entry(path, kind, cin, cout, hw, batch, want_name):
    """Both kinds of one (cin, cout, shape) on whichever kernel the library now picks."""
    tag = f"{cin}->{cout} {hw} b{batch}"
    assert kernels.conv2d_kernel_name(batch, cout, hw[0], hw[1], cin) == want_name, (tag, want_name)
    if kind == "int":
        c = J.conv2d_int(cin, cout, hw, batch)
        x, r = dev(c["x"]).unsqueeze(2), dev(c["r"]).unsqueeze(2)
        packed = kernels.pack_conv2d_weight(dev(c["w"]))
        raw = B.conv_raw(c["x"], c["w"], 3)
        for mode, (relu, res, acc) in MODES.items():
            got = run_conv2d(x, packed, cout, dev(c["scale"]), dev(c["shift"]), r, mode)
            judge_exact(path, f"{tag} {mode}", got, B.epilogue(raw, c["scale"], c["shift"], relu,
                                                               c["r"] if res or acc else None))
    else:
        j = J.conv2d_normal(cin, cout, hw, batch)
        got = run_conv2d(dev(j.x).unsqueeze(2), kernels.pack_conv2d_weight(dev(j.w)), cout, None, None, None,
                         "norelu")
        judge_scaled(path, tag, got, j.ref, j.s, j.e_model, j.bar, kernel=want_name)


@pytest.mark.parametrize("cin,cout", J.SMALL)
@pytest.mark.parametrize("kind", KINDS)
def test_small_kernel_every_instantiation(kind, cin, cout):
    """conv2d_small_kernel<CIN, NG> on 9 x 35 (a second 32-column tile 3 wide, a ragged row tile for
    TH = 8, 4 and 2) and 1 x 1; plain, residual, accumulate and no ReLU; couts that are no
    multiple of 8 (5, 12, 20) must leave the sentinel channels after them untouched."""
    with _lib.tuning(lea_conv2d_set_small=1):
        for hw, batch in J.SMALL_SHAPES:
            conv2d_entry("small", kind, cin, cout, hw, batch, small_name(cin, cout))


def test_small_cases_cover_all_twelve_instantiations():
    """The names the library reports for the cases above are the twelve of
    conv2d_small.hip:155-158 (each case asserts its own name before it launches)."""
    with _lib.tuning(lea_conv2d_set_small=1):
        names = {kernels.conv2d_kernel_name(2, cout, *J.HW_RAGGED, cin) for cin, cout in J.SMALL}
    assert names == {f"conv2d_small_kernel<{ci}, {ng}>" for ci in (4, 8, 12, 16) for ng in (1, 2, 4)}, names
    assert names == {small_name(cin, cout) for cin, cout in J.SMALL}


@pytest.mark.parametrize("cin,cout,hw,batch", sorted(J.DMA2D))
@pytest.mark.parametrize("kind", KINDS)
def test_dma2d_engine_every_tile(kind, cin, cout, hw, batch):
    """conv3d_dma_kernel<MT, NT, 16, 1, 1> with the few-channel tile off: mt 1 .. 4 (couts 16, 32,
    48, 64), several cout blocks (96: two of mt 3, 192: three of mt 4), the 4 x 16 tile on 9 x 35 /
    9 x 36 and the 8 x 16 tile on 123 x 250 at batch 2 (512 workgroups per cout block, the last
    row tile 3 high, the last column tile 10 wide)."""
    mt, nt = J.DMA2D[(cin, cout, hw, batch)]
    with _lib.tuning(lea_conv2d_set_small=0):
        conv2d_entry("dma2d", kind, cin, cout, hw, batch, dma2d_name(mt, nt))


def test_dma2d_cases_cover_all_eight_tiles():
    with _lib.tuning(lea_conv2d_set_small=0):
        names = {kernels.conv2d_kernel_name(b, cout, hw[0], hw[1], cin) for cin, cout, hw, b in J.DMA2D}
    assert names == {dma2d_name(mt, nt) for mt in (1, 2, 3, 4) for nt in (1, 2)}, names


# ------------------------------------------------------------------ the pair launch
@pytest.mark.parametrize("kind,cin,c1,cout,res", [(k,) + p + (r,) for k in KINDS for p in J.PAIR
                                                  for r in ((False, True) if k == "int" else (False,))])
def test_pair_launch_against_the_judge(kind, cin, c1, cout, res):
    """lea_conv2d_bnrelu_pair into two non-adjacent slots of one buffer, against the float64 judge
    of the stacked conv (not against the single-conv kernel); the residual joins the first c1
    couts only.  The normal kind is the pure conv, so the residual -- an epilogue -- is judged in
    the int kind, exactly."""
    hw, batch = J.HW_RAGGED, 2
    tag = f"{cin}->{c1}+{cout - c1} {'res' if res else 'plain'}"
    assert kernels.conv2d_kernel_name(batch, cout, hw[0], hw[1], cin) == small_name(cin, cout)
    buf = torch.full((batch, cout + 3 * PAD, 1) + hw, SENTINEL, device=DEV)
    out1, out2 = buf[:, PAD:PAD + c1], buf[:, 2 * PAD + c1:2 * PAD + cout]
    if kind == "int":
        c = J.conv2d_int(cin, cout, hw, batch)
        x, w, scale, shift = c["x"], c["w"], c["scale"], c["shift"]
        r = c["r"][:, :c1].contiguous() if res else None
    else:
        j = J.conv2d_normal(cin, cout, hw, batch)
        x, w, scale, shift, r = j.x, j.w, None, None, None
    kernels.conv2d_bnrelu_pair(dev(x).unsqueeze(2), kernels.pack_conv2d_weight(dev(w)), c1, cout,
                               None if scale is None else dev(scale), None if shift is None else dev(shift),
                               kind == "int", out1, out2, None if r is None else dev(r).unsqueeze(2))
    torch.cuda.synchronize()
    for lo, hi in ((0, PAD), (PAD + c1, 2 * PAD + c1), (2 * PAD + cout, 3 * PAD + cout)):
        assert bool((buf[:, lo:hi] == SENTINEL).all()), f"{tag}: channels {lo}:{hi} of the buffer were written"
    got = torch.cat((out1, out2), 1)[:, :, 0]
    if kind == "int":
        want = B.conv_judge(x, w, scale, shift, True, k=3)
        if res:
            want[:, :c1] += r.double()
        judge_exact("pair", tag, got, want)
    else:
        judge_scaled("pair", tag, got, j.ref, j.s, j.e_model, j.bar)


# ------------------------------------------------------------------ 3x3 / s3
def run_s3(x, w, scale, shift, relu):
    b, cin, _, hi, wi = x.shape
    cout = w.shape[0]
    s = SentinelF32(b, cout, (1, (hi - 1) // 3 + 1, (wi - 1) // 3 + 1))
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(_lib.load().lea_conv2d_s3_bnrelu(
        x.data_ptr(), x.stride(0), w.data_ptr(), ptr(scale), ptr(shift), s.out.data_ptr(), s.big.stride(0), b, cin,
        cout, hi, wi, _lib.LEA_RELU if relu else 0, _lib.LEA_F32, kernels._stream()), "lea_conv2d_s3_bnrelu")
    s.check()
    return s.out[:, :, 0]


@pytest.mark.parametrize("hw", J.S3_SHAPES)
@pytest.mark.parametrize("cin,cout", J.S3)
@pytest.mark.parametrize("kind", KINDS)
def test_stride3_conv(kind, cin, cout, hw):
    """lea_conv2d_s3_bnrelu with Hi mod 3 and Wi mod 3 each 0, 1 and 2, and 4 x 3 (every output on
    the padding); cout 20 ends in a partial block of 16 couts."""
    tag = f"{cin}->{cout} {hw}"
    if kind == "int":
        c = J.s3_int(cin, cout, hw)
        x, w, scale, shift = dev(c["x"]).unsqueeze(2), dev(c["w"]), dev(c["scale"]), dev(c["shift"])
        for relu in (True, False):
            judge_exact("s3", f"{tag} relu={relu}", run_s3(x, w, scale, shift, relu),
                        J.s3_judge(c["x"], c["w"], c["scale"], c["shift"], relu))
    else:
        j = J.conv2d_normal(cin, cout, hw, 2, 3)
        judge_scaled("s3", tag, run_s3(dev(j.x).unsqueeze(2), dev(j.w), None, None, False), j.ref, j.s, j.e_model,
                     j.bar)


# ------------------------------------------------------------------ fused stems
@pytest.mark.parametrize("hw", J.STEM_SHAPES)
@pytest.mark.parametrize("c8", [False, True], ids=["f32", "c8"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_stems(kind, c8, hw):
    """lea_feature_stem_bnrelu: Wo = 66 / 67 crosses the 64-column seam of its workgroup, Ho = 8 the
    4-row seam; 5 x 7: every output touches padding.  In the int kind shift0 is positive on several
    stem0 channels, so stem1's padding ring must read 0 and not relu(shift0)."""
    c = J.stem_case(kind, hw)
    batch, (hi, wi) = c["x"].shape[0], hw
    ho, wo = (hi - 1) // 3 + 1, (wi - 1) // 3 + 1
    s = (Sentinel if c8 else SentinelF32)(batch, J.STEM_C1, (1, ho, wo))
    x, w0, s0, t0, w1, s1, t1 = (dev(t) for t in J.stem_args(c))
    _lib.check(_lib.load().lea_feature_stem_bnrelu(
        x.data_ptr(), x.stride(0), w0.data_ptr(), s0.data_ptr(), t0.data_ptr(), w1.data_ptr(), s1.data_ptr(),
        t1.data_ptr(), s.out.data_ptr(), s.big.stride(0), batch, J.STEM_CIN, J.STEM_C0, J.STEM_C1, hi, wi,
        _lib.LEA_BF16 if c8 else _lib.LEA_F32, kernels._stream()), "lea_feature_stem_bnrelu")
    s.check()
    got = from_c8(s.out, 2) if c8 else s.out[:, :, 0].double().cpu()
    path, tag = "stems c8" if c8 else "stems f32", f"{hw}"
    if kind == "int":
        judge_exact(path, tag, got, c["want"])  # exact in bf16 as well (asserted on the reference)
    elif c8:
        judge_c8(path, tag, got, c["want"], c["e32"])
    else:
        assert torch.isfinite(got).all()
        d = (got - c["want"]).abs() / float(c["want"].abs().max())
        e, bar = float(d.max()), J.MARGIN * c["e_chain"]
        record(path, tag, kind, err=e, model=c["e_chain"], bar=bar, share=float((d > bar).double().mean()),
               used=e / c["e_chain"], n=got.numel())
        assert e <= bar, f"{path} {tag}: {e:.3e} of max |ref| > {bar:.3e} = {J.MARGIN} x the float32 chain"


# ------------------------------------------------------------------ factored stem0
def run_combine(lm, rm, cout, d3, scale, shift, relu, c8):
    """lea_cv_stem_combine into a sentinel-guarded slice; returns float64 NCDHW on the CPU."""
    b, h, w = lm.shape[0], lm.shape[3], lm.shape[4]
    assert kernels.cv_stem_supported(cout, d3, w, c8)
    s = (Sentinel if c8 else SentinelF32)(b, cout, (d3, h, w))
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(_lib.load().lea_cv_stem_combine(
        lm.data_ptr(), lm.stride(0), rm.data_ptr(), rm.stride(0), ptr(scale), ptr(shift), s.out.data_ptr(),
        s.big.stride(0), b, cout, d3, h, w, _lib.LEA_RELU if relu else 0, _lib.LEA_BF16 if c8 else _lib.LEA_F32,
        kernels._stream()), "lea_cv_stem_combine")
    s.check()
    return from_c8(s.out) if c8 else s.out.double().cpu()


def split_on_device(w):
    """lea_cv_stem_split_weights, which must equal the judge's restatement bit for bit."""
    wl, wr = kernels.cv_stem_split_weights(dev(w))
    jl, jr = J.split_weights(w)
    assert torch.equal(wl.cpu(), jl) and torch.equal(wr.cpu(), jr)
    return wl, wr


@pytest.mark.parametrize("c,cout,maxdisp,hw,batch", J.CV_F32)
@pytest.mark.parametrize("kind", KINDS)
def test_cv_stem_combine_f32(kind, c, cout, maxdisp, hw, batch):
    """lea_cv_stem_combine in f32 on maps from lea_conv2d_bnrelu: D3 = 9 > W = 8 (correction indices
    out of range), W = 64 exactly, 72 and 132 (two and three segments), couts 24 and 48, and
    D3 = 545, the smallest that splits the planes over two workgroups."""
    f = J.cv_case(kind, "f32", c, cout, maxdisp, hw, batch)
    d3 = maxdisp // 3
    tag = f"C{c}->{cout} md{maxdisp} {hw}"
    wl, wr = split_on_device(f["w"])
    lm = kernels.conv2d_bnrelu(dev(f["fl"]).unsqueeze(2), kernels.pack_conv2d_weight(wl), 9 * cout, None, None,
                               relu=False)
    rm = kernels.conv2d_bnrelu(dev(f["fr"]).unsqueeze(2), kernels.pack_conv2d_weight(wr), 6 * cout, None, None,
                               relu=False)
    if kind == "int":
        judge_exact("cv_stem f32", tag, run_combine(lm, rm, cout, d3, dev(f["scale"]), dev(f["shift"]), True, False),
                    f["want"])
    else:
        judge_scaled("cv_stem f32", tag, run_combine(lm, rm, cout, d3, None, None, False, False), f["ref"], f["s"],
                     max(f["e_comb"], f["e_direct"]), f["bar"], e_comb=f["e_comb"], e_direct=f["e_direct"])


@pytest.mark.parametrize("c,cout,maxdisp,hw,batch", J.CV_C8)
@pytest.mark.parametrize("kind", KINDS)
def test_cv_stem_combine_c8(kind, c, cout, maxdisp, hw, batch):
    """lea_cv_stem_combine in c8 on maps from lea_conv2d_bnrelu_bf16: odd W (19), cout 40 (a partial
    block of 32 couts), W = 70 (two segments) and D3 = 225, the smallest that splits the planes."""
    f = J.cv_case(kind, "c8", c, cout, maxdisp, hw, batch)
    d3 = maxdisp // 3
    tag = f"C{c}->{cout} md{maxdisp} {hw}"
    wl, wr = split_on_device(f["w"])
    lm = kernels.conv2d_bnrelu_bf16(to_c8(f["fl"]), kernels.pack_conv2d_weight_bf16(wl), 9 * cout, None, None,
                                    relu=False)
    rm = kernels.conv2d_bnrelu_bf16(to_c8(f["fr"]), kernels.pack_conv2d_weight_bf16(wr), 6 * cout, None, None,
                                    relu=False)
    got = run_combine(lm, rm, cout, d3, dev(f["scale"]), dev(f["shift"]), True, True)
    if kind == "int":
        judge_exact("cv_stem c8", tag, got, f["want"])
        return
    lm64, rm64 = from_c8(lm, 2), from_c8(rm, 2)
    judge_c8("cv_stem c8 maps", tag + " left", lm64, f["lm"], f["e32_maps"])
    judge_c8("cv_stem c8 maps", tag + " right", rm64, f["rm"], f["e32_maps"])
    want = J.stem0_from_maps(lm64, rm64, cout, d3, f["scale"], f["shift"])
    e32 = J.stem0_c8_e32(lm64, rm64, cout, d3, f["scale"], f["shift"])
    moved = int((B.half_ulp_stats(got, f["want"], f["e32"])["share"]) * got.numel() + 0.5)
    judge_c8("cv_stem c8", tag, got, want, e32, moved=moved)
