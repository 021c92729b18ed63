"""The bf16 conv engine (csrc/conv3d_bf16.hip) against the fp64 judge of tests/bf16_judge.py
on every dispatch path: each instantiated tile of conv_bf16_kernel (through
lea_conv3d_bf16_set_tile_override), the planner's D-streaming kernel, the pair launch on both
of its kernels, the streamed 1x1 walking several tiles per wave, the cost-volume entry and
the 2D entry with th = 8.

Every case runs twice.  "int": the integer recipe, on which every sum and rounding point is
exact (asserted on the reference), so the output must EQUAL rn_bf16(judge) bit for bit -- a
wrong tap, channel, halo, block or store cannot hide.  "normal": the N(0, 1) recipe of
tests/test_gpu_bf16.py under assert_half_ulp: every element within half a bf16 ulp + 4 e32
of the fp64 value, e32 that case's float32-on-CPU distance from fp64; truncation, a double
rounding or a bf16 partial sum fail it on 3-25 % of the elements (tests/
test_bf16_judge_cpu.py).  The pair launch is judged with the rounding of the kernel it runs
(bf16_judge.pair_rounds_a): conv a's activation rounded to bf16 first on the split-wave pair
kernel, one rounding of the f32 sum on the D-streaming kernel.

Outputs go into a block slice between two sentinel blocks, the launch's kernel is asserted
through kernels.conv_kernel_name_bf16 (the 2D entry and the 1x1 walk, which have no name
query, by recomputing the entry's own formula), every setter is restored, references are
computed once per case.  Each case prints its figures (pytest -s): the share of failing
elements, and "used" = the worst (|got - fp64| - half ulp) / e32, which the margin 4 has to
cover.

Measured on an MI355X with the margin at 4 (no case needed more; no failing element and, on
the integer recipe, no differing element on any path).  Worst "used" per path, e32 being
3e-7 .. 3e-6 throughout:

    path                                   launches   worst used   at
    tile kernel, 3D (every override)          234        0.51      64->96 th4 td1 mt1 acc
    tile kernel, k = 1 (every override)        36        0.18      24->8 th4 mt1 res
    tile kernel, planner's pick at D = 3        6        0.07      32->32 acc
    D-streaming kernel                         30        0.20      32->32 (33, 9, 20) acc
    pair launch on conv_bf16_pair_kernel       10        1.51      c8 (9, 12, 33) split 1
    pair launch on the D-streaming kernel       6        0.11      c16 (9, 12, 33) split 0
    streamed 1x1, tpw = 2                       5        0.23      24->8 acc
    cost-volume entry                          26        0.88      C32->32 md48, planner's tile
    2D entry                                    9        0.16      16->96 (130, 260) res

Refused overrides: exactly REFUSED below (td = 4 on the cost-volume entry, td > 1 at k = 1).
"""
import functools
import json

import pytest
import torch

from leastereo_amd import _lib, kernels
from tests import bf16_judge as J

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.0
KINDS = ("int", "normal")
UNSUPPORTED = "rc=1002"  # LEA_E_UNSUPPORTED (include/leastereo_hip.h), as _lib.check words it

# Override combinations the library refuses with LEA_E_UNSUPPORTED (run(): the instantiation
# lists LEA_BF_MT at conv3d_bf16.hip:1373-1384), as (entry, th, td, mt); every other
# combination of th {4, 8, 16} x td {1, 2, 4} x mt {1, 2} must launch.  A tile that
# disappears later fails its own case; one that appears fails test_refused_overrides.
REFUSED = ({("costvolume", th, 4, mt) for th in (4, 8, 16) for mt in (1, 2)}
           | {("k1", th, td, mt) for th in (4, 8, 16) for td in (2, 4) for mt in (1, 2)})


def to_c8(t):
    """bf16-exact f32 [B, C, (D,) H, W] on the CPU -> c8 on the device, by torch alone."""
    b, c = t.shape[:2]
    sp = tuple(t.shape[2:]) if t.dim() == 5 else (1,) + tuple(t.shape[2:])
    y = t.reshape(b, c // 8, 8, *sp).permute(0, 1, 3, 4, 5, 2).contiguous()
    assert torch.equal(y.to(torch.bfloat16).float(), y)
    return y.to(torch.bfloat16).to(DEV)


def from_c8(y, nd=3):
    b, cb, d, h, w, _ = y.shape
    t = y.permute(0, 1, 5, 2, 3, 4).reshape(b, cb * 8, d, h, w).double().cpu()
    return t if nd == 3 else t[:, :, 0]


def record(path, tag, kind, st):
    """One JSON line per launch on stdout (pytest -s)."""
    print(json.dumps(dict(path=path, case=tag, kind=kind, **st)))


def judge(path, tag, kind, got, want, e32, alts=()):
    if kind == "int":
        J.assert_bf16_exact(want, tag)
        bad = int((got != want).sum())
        record(path, tag, kind, dict(mismatches=bad, n=got.numel()))
        assert torch.equal(got, want), f"{tag}: {bad} of {got.numel()} elements differ from the exact result"
    else:
        try:
            st = J.assert_half_ulp(got, want, e32, alts, tag=tag)
        except AssertionError:
            record(path, tag, kind, J.half_ulp_stats(got, want, e32, alts))
            raise
        record(path, tag, kind, st)


class Sentinel:
    """An output block slice between two sentinel blocks."""

    def __init__(self, b, cout, vol):
        self.big = torch.full((b, cout // 8 + 2) + tuple(vol) + (8,), SENTINEL, device=DEV, dtype=torch.bfloat16)
        self.out = self.big[:, 1:1 + cout // 8]

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.big[:, 0] == SENTINEL).all()) and bool((self.big[:, -1] == SENTINEL).all()), \
            "a neighbouring block was written"


# mode -> (relu, uses the residual operand)
MODES = {"plain": (True, False), "res": (True, True), "acc": (False, True)}


@functools.lru_cache(maxsize=6)
def conv_case(kind, cin, cout, k, shape, b=2):
    """Per case, computed once and left unchanged: operands (CPU and device), per epilogue
    mode the fp64 judge and e32."""
    seed = cin * 13 + cout + k + sum(shape)
    c = (J.integer_case if kind == "int" else J.normal_case)(seed, cin, cout, k, shape, b)
    raw64, raw32 = J.conv_raw(c["x"], c["w"], k), J.conv_raw(c["x"], c["w"], k, torch.float32)
    want, e32 = {}, {}
    for mode, (relu, res) in MODES.items():
        want[mode] = J.epilogue(raw64, c["scale"], c["shift"], relu, c["r"] if res else None)
        e32[mode] = J.e32_of(J.epilogue(raw32, c["scale"], c["shift"], relu, c["r"] if res else None), want[mode])
    nd = len(shape)
    w_dev = c["w"].to(DEV)
    packed = kernels.pack_conv_weight_bf16(w_dev) if nd == 3 else kernels.pack_conv2d_weight_bf16(w_dev)
    return dict(c, want=want, e32=e32, xc=to_c8(c["x"]), rc=to_c8(c["r"]), packed=packed,
                scale_d=c["scale"].to(DEV), shift_d=c["shift"].to(DEV), vol=shape if nd == 3 else (1,) + shape)


def run_conv(case, cout, k, mode, cin2=0):
    """One launch of the 3D entry into a sentinel-guarded block slice; returns f64 NCDHW."""
    relu, res = MODES[mode]
    xc = case["xc"]
    s = Sentinel(xc.shape[0], cout, case["vol"])
    if mode == "acc":
        s.out.copy_(case["rc"])
    x1, x2 = (xc[:, :-(cin2 // 8)], xc[:, -(cin2 // 8):]) if cin2 else (xc, None)
    kernels.conv3d_bnrelu_bf16(x1, case["packed"], cout, k, case["scale_d"], case["shift_d"], relu=relu,
                               out=s.out, accumulate=mode == "acc", x2=x2,
                               residual=case["rc"] if mode == "res" else None)
    s.check()
    return from_c8(s.out)


def tile_name(cin, cout, k, th, td, mt, cv=False):
    cobv = 16 if cout <= 16 else (32 if cout <= 32 else 64)
    mt = min(mt, cobv // 16)
    nb = 4 if k == 1 else (1 if cin <= 8 else 2)
    return f"conv_bf16_kernel<{k}, {mt}, {cobv // 16 // mt}, {th}, {td}, {nb}, {'true' if cv else 'false'}>"


# ------------------------------------------------------------- a. every instantiated tile
VOL_A = (5, 19, 37)  # ragged against 16 columns and th 4 / 8 / 16; odd D partial for td 2, 4
TILES = [(th, td, mt) for th in (4, 8, 16) for td in (1, 2, 4) for mt in (1, 2)]


@pytest.mark.parametrize("th,td,mt", TILES)
@pytest.mark.parametrize("cin,cout", [(8, 8), (16, 32), (32, 64), (64, 96)])
@pytest.mark.parametrize("kind", KINDS)
def test_tile_kernel_every_tile(kind, cin, cout, th, td, mt):
    """conv_bf16_kernel<3, MT, WC, TH, TD, NB>: nb 1 (8 -> 8), nb 2 with (mt, wc) = (1, 2) /
    (2, 1) (16 -> 32), two chunks with (1, 4) / (2, 2) (32 -> 64), two cout blocks, the last
    short (64 -> 96; once as two 32-channel sources); plain, residual and accumulate."""
    lib = _lib.load()
    case = conv_case(kind, cin, cout, 3, VOL_A)
    assert ("k3", th, td, mt) not in REFUSED
    with _lib.tuning(lea_conv3d_bf16_set_tile_override=(th, td, mt)):
        assert kernels.conv_kernel_name_bf16(2, cout, cin, *VOL_A, 3) == tile_name(cin, cout, 3, th, td, mt)
        runs = [(m, 0) for m in MODES] + ([("plain", 32)] if cin == 64 else [])
        outs = [(m, c2, run_conv(case, cout, 3, m, c2)) for m, c2 in runs]
    for mode, c2, got in outs:
        judge("tile", f"{cin}->{cout} th{th} td{td} mt{mt} {mode}{' x2' if c2 else ''}", kind, got,
              case["want"][mode], case["e32"][mode])


@pytest.mark.parametrize("th,mt", [(th, mt) for th in (4, 8, 16) for mt in (1, 2)])
@pytest.mark.parametrize("cin,cout", [(24, 8), (128, 64)])
@pytest.mark.parametrize("kind", KINDS)
def test_tile_kernel_1x1_every_tile(kind, cin, cout, th, mt):
    """The k = 1 tile kernel (the streamed 1x1 off): a padded chunk (24 -> 8), four chunks
    with (mt, wc) = (1, 4) / (2, 2) (128 -> 64)."""
    lib = _lib.load()
    case = conv_case(kind, cin, cout, 1, VOL_A)
    with _lib.tuning(lea_conv3d_bf16_set_stream1x1=0, lea_conv3d_bf16_set_tile_override=(th, 1, mt)):
        assert kernels.conv_kernel_name_bf16(2, cout, cin, *VOL_A, 1) == tile_name(cin, cout, 1, th, 1, mt)
        outs = [(m, run_conv(case, cout, 1, m)) for m in MODES]
    for mode, got in outs:
        judge("tile 1x1", f"{cin}->{cout} th{th} mt{mt} {mode}", kind, got, case["want"][mode], case["e32"][mode])


def test_refused_overrides():
    """Exactly the combinations of REFUSED answer LEA_E_UNSUPPORTED, before any launch."""
    lib = _lib.load()
    k1 = conv_case("int", 24, 8, 1, (4, 3, 5))
    cv = costvolume_case("int", 16, 16, 27, (5, 19))
    for entry, th, td, mt in sorted(REFUSED):
        with _lib.tuning(lea_conv3d_bf16_set_tile_override=(th, td, mt)):
            with pytest.raises(_lib.HipKernelError, match=UNSUPPORTED):
                if entry == "k1":
                    run_conv(k1, 8, 1, "plain")
                else:
                    kernels.conv3d_bnrelu_costvolume_bf16(cv["flc"], cv["frc"], 27, cv["packed"], 16,
                                                          cv["scale_d"], cv["shift_d"])
    assert lib.lea_conv3d_bf16_set_tile_override(12, 2, 1) == _lib.LEA_E_INVALID  # no such tile at all
    assert lib.lea_conv3d_bf16_set_tile_override(0, 0, 0) == 0


# --------------------------------------------------------------------- b. planner defaults
@pytest.mark.parametrize("cin,cout,shape", [
    (cin, cout, shape) for cin, cout in [(8, 8), (16, 16), (32, 32), (8, 24), (16, 48)]
    for shape in [(33, 9, 20), (4, 3, 5)]] + [(8, 8, (3, 9, 20)), (32, 32, (3, 9, 20))])
@pytest.mark.parametrize("kind", KINDS)
def test_planner_default_paths(kind, cin, cout, shape):
    """What the planner picks at small size: the D-streaming kernel (odd D with several
    column segments along D; the smallest streamed depth) and, at D = 3, the tile kernel."""
    case = conv_case(kind, cin, cout, 3, shape)
    name = kernels.conv_kernel_name_bf16(2, cout, cin, *shape, 3)
    assert name.startswith("conv_bf16_stream_kernel<" if shape[0] >= 4 else "conv_bf16_kernel<3,"), name
    for mode in MODES:
        judge("stream" if shape[0] >= 4 else "tile (planner)", f"{cin}->{cout} {shape} {mode}", kind,
              run_conv(case, cout, 3, mode), case["want"][mode], case["e32"][mode])


# --------------------------------------------------------------------------- c. pair launch
@functools.lru_cache(maxsize=4)
def pair_case(kind, c, shape):
    seed = c * 3 + shape[0]
    p = (J.integer_pair_case if kind == "int" else J.normal_pair_case)(seed, c, shape)
    args = (p["xa"], p["wa"], p["xb"], p["wb"], p["sc"], p["sh"])
    a64, b64 = J.pair_terms(*args)
    e32 = J.e32_of(J.pair_judge(*args, False, dtype=torch.float32), a64 + b64)
    packed = torch.cat([kernels.pack_conv_weight_bf16(p["wa"].to(DEV)), kernels.pack_conv_weight_bf16(p["wb"].to(DEV))])
    return dict(a64=a64, b64=b64, e32=e32, xa=to_c8(p["xa"]), xb=to_c8(p["xb"]), packed=packed,
                sc=p["sc"].to(DEV), sh=p["sh"].to(DEV))


@pytest.mark.parametrize("split", [0, 1, 2, 3])
@pytest.mark.parametrize("c,shape", [(c, s) for c in (8, 16) for s in [(9, 12, 33), (4, 4, 16)]])
@pytest.mark.parametrize("kind", KINDS)
def test_pair_launch_rounds_as_its_kernel(kind, c, shape, split):
    """LEA_PAIR_SUM: two roundings on conv_bf16_pair_kernel, one on the D-streaming kernel;
    which of them runs follows run() from the plan asserted here and the split."""
    lib = _lib.load()
    case = pair_case(kind, c, shape)
    round_a = J.pair_rounds_a(c, split)
    s = Sentinel(2, c, shape)
    assert kernels.pair_sum_supported_bf16(case["xa"], case["xb"], s.out)
    th, nb = (8, 1) if c == 8 else (4, 2)
    assert kernels.conv_kernel_name_bf16(2, c, c, *shape, 3) == f"conv_bf16_stream_kernel<1, 1, {th}, {nb}, 1>"
    with _lib.tuning(lea_conv3d_bf16_set_pair_split=split):
        kernels.conv3d_bnrelu_bf16(case["xa"], case["packed"], c, 3, case["sc"], case["sh"], True, s.out,
                                   x2=case["xb"], pair_sum=True)
        s.check()
    want, alts = J.pair_wants(case["a64"], case["b64"], case["e32"], round_a)
    got = from_c8(s.out)
    judge("pair kernel" if round_a else "pair on stream", f"c{c} {shape} split{split}", kind, got, want,
          case["e32"], alts)
    if kind == "normal":
        # ... and not as the other kernel: the float32 restatement rounded the other way misses on
        # 3 % of the elements (tests/test_bf16_judge_cpu.py, which asserts more than 0.1 %)
        other, oalts = J.pair_wants(case["a64"], case["b64"], case["e32"], not round_a)
        assert J.half_ulp_stats(got, other, case["e32"], oalts)["share"] > 1e-3


# ----------------------------------------------------------- d. streamed 1x1, tpw > 1
VOL_D = (23, 47, 81)  # 5473 tiles of 16 voxels, the last partial; not a multiple of 8 tiles


@pytest.mark.parametrize("cin,cout,mode,cin2", [(32, 32, "plain", 0), (64, 32, "res", 0), (64, 32, "plain", 32),
                                                 (128, 64, "plain", 0), (24, 8, "acc", 0)])
@pytest.mark.parametrize("kind", KINDS)
def test_stream_1x1_several_tiles_per_wave(kind, cin, cout, mode, cin2):
    """conv1x1_c8_kernel with tpw = 2: the multi-tile walk and its partial last group."""
    case = conv_case(kind, cin, cout, 1, VOL_D)
    vox = VOL_D[0] * VOL_D[1] * VOL_D[2]
    tiles, ncob = (vox + 15) // 16, (cout + 63) // 64
    tpw = max(1, (tiles * 2 * ncob + 8191) // 8192)  # run(), conv3d_bf16.hip:1325
    assert tpw >= 2 and tiles % 8 != 0 and vox % 16 != 0
    assert kernels.conv_kernel_name_bf16(2, cout, cin, *VOL_D, 1).startswith("conv1x1_c8_kernel<")
    judge("streamed 1x1", f"{cin}->{cout} {mode}{' x2' if cin2 else ''}", kind,
          run_conv(case, cout, 1, mode, cin2), case["want"][mode], case["e32"][mode])


# ------------------------------------------------------------------ e. cost-volume entry
@functools.lru_cache(maxsize=4)
def costvolume_case(kind, c, cout, maxdisp, hw):
    f = (J.integer_costvolume_case if kind == "int" else J.normal_costvolume_case)(c + maxdisp, c, cout, maxdisp, hw)
    want = J.costvolume_judge(f["fl"], f["fr"], maxdisp, f["w"], f["scale"], f["shift"], True)
    e32 = J.e32_of(J.costvolume_judge(f["fl"], f["fr"], maxdisp, f["w"], f["scale"], f["shift"], True,
                                      dtype=torch.float32), want)
    return dict(want=want, e32=e32, flc=to_c8(f["fl"]), frc=to_c8(f["fr"]),
                packed=kernels.pack_conv_weight_bf16(f["w"].to(DEV)), scale_d=f["scale"].to(DEV),
                shift_d=f["shift"].to(DEV))


@pytest.mark.parametrize("th,td,mt", [(0, 0, 0)] + [(th, td, mt) for th in (4, 8, 16) for td in (1, 2) for mt in (1, 2)])
@pytest.mark.parametrize("c,cout,maxdisp,hw", [(16, 16, 27, (5, 19)), (32, 32, 48, (12, 40))])
@pytest.mark.parametrize("kind", KINDS)
def test_costvolume_entry(kind, c, cout, maxdisp, hw, th, td, mt):
    """lea_conv3d_bnrelu_costvolume_bf16 (the volume never built: zero where w < d) against
    the judge's explicit volume; the planner's tile (0, 0, 0) and every override."""
    lib = _lib.load()
    case = costvolume_case(kind, c, cout, maxdisp, hw)
    d3 = maxdisp // 3
    assert ("costvolume", th, td, mt) not in REFUSED
    with _lib.tuning(lea_conv3d_bf16_set_tile_override=(th, td, mt)):
        name = kernels.conv_kernel_name_bf16(2, cout, 2 * c, d3, *hw, 3, True)
        if th:
            assert name == tile_name(2 * c, cout, 3, th, td, mt, cv=True)
        assert name.startswith("conv_bf16_kernel<3,") and name.endswith("true>"), name
        got = kernels.conv3d_bnrelu_costvolume_bf16(case["flc"], case["frc"], maxdisp, case["packed"], cout,
                                                    case["scale_d"], case["shift_d"])
        torch.cuda.synchronize()
    judge("cost volume", f"C{c}->{cout} md{maxdisp} {hw} th{th} td{td} mt{mt}", kind, from_c8(got), case["want"],
          case["e32"])


# ------------------------------------------------------------------------- f. the 2D entry
@pytest.mark.parametrize("cin,cout,hw,th", [(8, 8, (250, 330), 8), (16, 96, (130, 260), 8), (8, 8, (19, 33), 4)])
@pytest.mark.parametrize("kind", KINDS)
def test_conv2d_entry(kind, cin, cout, hw, th):
    """lea_conv2d_bnrelu_bf16: th = 8 is picked from 1024 workgroups on (the entry's wgs8
    formula, recomputed here); ragged H and W; every epilogue."""
    case = conv_case(kind, cin, cout, 3, hw)
    h, w = hw
    ncob = (cout + 63) // 64 if cout > 32 else 1
    wgs8 = ((w + 15) // 16) * ((h + 7) // 8) * 2 * ncob  # lea_conv2d_bnrelu_bf16, conv3d_bf16.hip:1782
    assert (wgs8 >= 1024) == (th == 8) and h % 8 and w % 16
    for mode, (relu, res) in MODES.items():
        s = Sentinel(2, cout, (1,) + hw)
        if mode == "acc":
            s.out.copy_(case["rc"])
        kernels.conv2d_bnrelu_bf16(case["xc"], case["packed"], cout, case["scale_d"], case["shift_d"], relu=relu,
                                   out=s.out, accumulate=mode == "acc",
                                   residual=case["rc"] if mode == "res" else None)
        s.check()
        judge("2D", f"{cin}->{cout} {hw} th{th} {mode}", kind, from_c8(s.out, 2), case["want"][mode],
              case["e32"][mode])
