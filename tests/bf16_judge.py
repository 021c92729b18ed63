"""The judge of the bf16 conv engine's per-op tests (CPU only, torch, float64 unless a dtype
is asked for; nothing here is taken from a kernel).

What the engine computes (``leastereo_amd/csrc/conv3d_bf16.hip``): bf16 operands, exact
products, f32 sums, the epilogue ``relu(conv * scale + shift) (+ residual)`` in f32
(``:241-254``; ``accumulate`` is the residual case with ``out`` as the residual) and ONE
rounding to bf16 at the store.  The judges return the **unrounded** value; two checks hang
a kernel's output on it:

* ``assert_half_ulp``: every element within half a bf16 ulp (one correct rounding) plus
  ``MARGIN * e32`` of the fp64 value, ``e32`` being the max abs distance of the same judge
  run in float32 on the CPU from the fp64 one on that very case (the f32 accumulation; the
  margin 4 for another summation order as in ``tests/test_gpu_disp_stats.py``).
* ``integer_case``: operands for which every sum and every rounding point is exact in
  bf16, so a correct kernel returns ``rn_bf16(judge)`` bit for bit, whatever its order.

The pair launch (LEA_PAIR_SUM: ``relu(BN_a(conv_a(xa))) + relu(BN_b(conv_b(xb)))``) rounds
differently per kernel, decided in ``run()`` (``conv3d_bf16.hip:1343-1360``): the split-wave
``conv_bf16_pair_kernel`` runs when ``g_pair_split != 0`` and the plan (``plan()``
``:1273-1285``: th = 8, nb = 1 for c = 8; th = 4, nb = 2 for c = 16) satisfies
``(nb == 2 && th == 4 && split != 3) || (nb == 1 && th == 8)`` (``:1344``); it stores conv
a's activation to LDS as bf16 (``:1200``) and rounds the sum again (``:1145``).  Everything
else falls through to the D-streaming kernel (``:1362-1368``), which sums in f32 and rounds
once (``:960-971``).  So ``round_a`` (``pair_rounds_a``) is

    channels | split 0 | split 1 | split 2 | split 3
    c = 8    | stream  | pair    | pair    | pair
    c = 16   | stream  | pair    | pair    | stream
"""
import torch
import torch.nn.functional as F

MARGIN = 4          # x e32: another summation order (tests/test_gpu_disp_stats.py)
BF16_MIN_EXP = -126  # smallest normal bf16 is 2^-126; spacing below it stays 2^-133


def _exponent(t64):
    """floor(log2 |t|), clamped at the smallest normal exponent (0 and subnormals there)."""
    _, e = torch.frexp(t64.abs())  # |t| = m 2^e, m in [0.5, 1)
    e = torch.where(t64 == 0, torch.full_like(e, BF16_MIN_EXP), e - 1)  # frexp(0) = (0, 0)
    return e.clamp_min(BF16_MIN_EXP)


def ulp_bf16(t64):
    """The bf16 spacing at |t|: 2^(floor(log2 |t|) - 7) (8 significant bits)."""
    t64 = t64.double()
    return torch.ldexp(torch.ones_like(t64), _exponent(t64) - 7)


def rn_bf16(t64):
    """Round to nearest, ties to even, to bf16 -- from the float64 value directly (no
    float32 in between, so no double rounding) -- returned as float64."""
    t64 = t64.double()
    u = ulp_bf16(t64)
    return torch.round(t64 / u) * u  # torch.round: halves to even; t / u is exact (u = 2^n)


def trunc_bf16(t64):
    """Toward zero to bf16 (the wrong rounding a test must reject), as float64."""
    t64 = t64.double()
    u = ulp_bf16(t64)
    return torch.trunc(t64 / u) * u


def conv_raw(x, w, k, dtype=torch.float64):
    """The plain convolution, 'same' zero padding: x [B, C, D, H, W] with w [O, C, k, k, k],
    or x [B, C, H, W] with w [O, C, k, k]."""
    x, w = x.to(dtype), w.to(dtype)
    return (F.conv3d if x.dim() == 5 else F.conv2d)(x, w, None, 1, k // 2)


def epilogue(raw, scale, shift, relu, residual=None):
    """relu(raw * scale + shift) (+ residual), unrounded, in raw's dtype."""
    dtype, bc = raw.dtype, (1, -1) + (1,) * (raw.dim() - 2)
    v = raw
    if scale is not None:
        v = v * scale.to(dtype).view(bc) + shift.to(dtype).view(bc)
    if relu:
        v = torch.relu(v)
    if residual is not None:
        v = v + residual.to(dtype)
    return v


def conv_judge(x, w, scale, shift, relu, residual=None, k=3, dtype=torch.float64):
    """The unrounded ConvBR value, 3D or 2D by x's rank: relu(conv * scale + shift) (+ residual)."""
    return epilogue(conv_raw(x, w, k, dtype), scale, shift, relu, residual)


def pair_terms(xa, wa, xb, wb, sc, sh, dtype=torch.float64):
    """The two unrounded activations of a pair launch: sc / sh hold conv a's c values, then
    conv b's; both ReLU'd (the matching-cell step)."""
    c = wa.shape[0]
    return (conv_judge(xa, wa, sc[:c], sh[:c], True, dtype=dtype),
            conv_judge(xb, wb, sc[c:], sh[c:], True, dtype=dtype))


def pair_rounds_a(c, split):
    """Whether the pair launch of c -> c channels under lea_conv3d_bf16_set_pair_split(split)
    runs conv_bf16_pair_kernel (two roundings); the table of the module docstring."""
    assert c in (8, 16) and split in (0, 1, 2, 3)
    return split != 0 and (c == 8 or split != 3)


def pair_judge(xa, wa, xb, wb, sc, sh, round_a, dtype=torch.float64):
    """round_a: rn_bf16(relu(BN_a(conv_a))) + relu(BN_b(conv_b)); else the plain sum."""
    a, b = pair_terms(xa, wa, xb, wb, sc, sh, dtype)
    return (rn_bf16(a).to(dtype) if round_a else a) + b


def pair_wants(a64, b64, e32, round_a):
    """The pair launch's acceptable unrounded values: the judge's, and with round_a the two it
    takes when conv a's activation sits within MARGIN * e32 of a rounding tie (there the
    kernel's f32 sum may round a the other way, a whole ulp apart, and both are correct).
    For the same reason a pair case's e32 is taken from the plain sum (round_a=False): a
    float32 restatement that flips one such tie would report a whole bf16 ulp as its error."""
    if not round_a:
        return a64 + b64, ()
    m = MARGIN * e32
    return rn_bf16(a64) + b64, (rn_bf16(a64 + m) + b64, rn_bf16(a64 - m) + b64)


def build_cost_volume(fl, fr, maxdisp, dtype=torch.float64):
    """[B, C, H, W] x 2 -> [B, 2C, maxdisp // 3, H, W]: plane d holds left(w) and right(w - d),
    zero where w < d."""
    b, c, h, w = fl.shape
    d3 = maxdisp // 3
    vol = torch.zeros(b, 2 * c, d3, h, w, dtype=dtype)
    for d in range(d3):
        if d < w:
            vol[:, :c, d, :, d:] = fl[..., d:].to(dtype)
            vol[:, c:, d, :, d:] = fr[..., :w - d].to(dtype)
    return vol


def costvolume_judge(fl, fr, maxdisp, w, scale, shift, relu, dtype=torch.float64):
    return conv_judge(build_cost_volume(fl, fr, maxdisp, dtype), w, scale, shift, relu, k=3, dtype=dtype)


def e32_of(j32, j64):
    return float((j32.double() - j64).abs().max())


def half_ulp_stats(got, want64, e32, alts=(), margin=MARGIN):
    """Per element the excess |got - want| - (0.5 ulp_bf16(max(|got|, |want|)) + margin e32),
    the smallest over want64 and the alternatives; no element is left out.  Returns the share
    of elements with a positive excess, the worst excess, that over e32, and the worst
    (|got - want| - 0.5 ulp) / e32 (what the margin has to cover; at most ``margin`` when
    the case passes)."""
    got = got.double().cpu()
    assert torch.isfinite(got).all()
    over = None
    for want in (want64,) + tuple(alts):
        want = want.double().cpu()
        assert want.shape == got.shape, (want.shape, got.shape)
        o = (got - want).abs() - 0.5 * ulp_bf16(torch.maximum(got.abs(), want.abs()))
        over = o if over is None else torch.minimum(over, o)
    excess = float((over - margin * e32).max())
    return dict(share=float((over > margin * e32).double().mean()), excess=excess,
                excess_over_e32=excess / max(e32, 1e-300), used_margin=float(over.max()) / max(e32, 1e-300),
                e32=e32, n=got.numel())


def assert_half_ulp(got, want64, e32, alts=(), margin=MARGIN, tag=""):
    """Fails unless EVERY element satisfies
        |got - want64| <= 0.5 ulp_bf16(max(|got|, |want64|)) + margin e32
    (against want64 or one of ``alts``, see pair_wants).  Under ReLU a fp64 value negative by
    more than margin e32 thereby demands an exact 0.  Prints the share of failing elements,
    the worst excess and that excess over e32 before it raises; returns the figures."""
    st = half_ulp_stats(got, want64, e32, alts, margin)
    if st["share"] > 0:
        print(f"{tag} half-ulp FAILED: share {st['share']:.3e} of {st['n']}, worst excess {st['excess']:.3e}, "
              f"excess / e32 {st['excess_over_e32']:.3e} (e32 {e32:.3e})")
        raise AssertionError(f"{tag}: {st}")
    return st


# ------------------------------------------------------------------------------ recipes
def bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def normal_case(seed, cin, cout, k, shape, batch=2):
    """The N(0, 1) recipe of tests/test_gpu_bf16.py: bf16-rounded activations, weights
    / sqrt(cin k^n), residual; scale in 0.5-1.5, shift 0.1 N."""
    g = torch.Generator().manual_seed(seed)
    nd = len(shape)
    x = bf(torch.randn((batch, cin) + tuple(shape), generator=g))
    w = bf(torch.randn((cout, cin) + (k,) * nd, generator=g) / float(cin * k ** nd) ** 0.5)
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    r = bf(torch.randn((batch, cout) + tuple(shape), generator=g))
    return dict(x=x, w=w, scale=scale, shift=shift, r=r)


def _ternary(g, shape, p):
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * (torch.rand(shape, generator=g) < p).float()


def assert_bf16_exact(t64, what=""):
    assert torch.equal(rn_bf16(t64), t64.double()), f"{what}: not exact in bf16 (max |v| {float(t64.abs().max())})"


def integer_case(seed, cin, cout, k, shape, batch=2):
    """Inputs on which every path is exact: activations in {-1, 0, 1} (non-zero with
    probability 0.5), weights in {-1, 0, 1} (0.25), scale in {0.5, 1, 2}, shift an integer in
    [-4, 4], residual an integer in [-8, 8].  Asserts ON THE REFERENCE ALONE that the value at
    every rounding point -- the activation with and without ReLU (also conv a's in a pair
    launch), and each with the residual added -- is unchanged by rn_bf16; the products are
    +-1 and the partial sums integers below 2^24, exact in f32 in any order.  So a correct
    kernel returns rn_bf16(judge) = judge bit for bit."""
    g = torch.Generator().manual_seed(seed)
    nd = len(shape)
    x = _ternary(g, (batch, cin) + tuple(shape), 0.5)
    w = _ternary(g, (cout, cin) + (k,) * nd, 0.25)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=g)]
    shift = torch.randint(-4, 5, (cout,), generator=g).float()
    r = torch.randint(-8, 9, (batch, cout) + tuple(shape), generator=g).float()
    case = dict(x=x, w=w, scale=scale, shift=shift, r=r)
    assert_integer_exact(conv_raw(x, w, k), scale, shift, r)
    return case


def assert_integer_exact(raw64, scale, shift, r):
    assert float(raw64.abs().max()) < 2 ** 24
    for relu in (True, False):
        v = epilogue(raw64, scale, shift, relu)
        assert_bf16_exact(v, f"activation relu={relu}")
        assert_bf16_exact(v + r.double(), f"activation + residual relu={relu}")


def integer_pair_case(seed, c, shape, batch=2):
    """integer_case for a pair launch: two c -> c convs; conv a's activation, conv b's and
    their sum all exact in bf16 (asserted on the reference)."""
    a = integer_case(seed, c, c, 3, shape, batch)
    b = integer_case(seed + 1000, c, c, 3, shape, batch)
    case = dict(xa=a["x"], wa=a["w"], xb=b["x"], wb=b["w"], sc=torch.cat((a["scale"], b["scale"])),
                sh=torch.cat((a["shift"], b["shift"])))
    ta, tb = pair_terms(case["xa"], case["wa"], case["xb"], case["wb"], case["sc"], case["sh"])
    for t, what in ((ta, "conv a"), (tb, "conv b"), (ta + tb, "sum")):
        assert_bf16_exact(t, what)
    return case


def normal_pair_case(seed, c, shape, batch=2):
    """The N(0, 1) recipe of test_pair_sum_bf16_vs_torch."""
    g = torch.Generator().manual_seed(seed)
    xa = bf(torch.randn((batch, c) + tuple(shape), generator=g))
    xb = bf(torch.randn((batch, c) + tuple(shape), generator=g))
    wa = bf(torch.randn(c, c, 3, 3, 3, generator=g) / float(c * 27) ** 0.5)
    wb = bf(torch.randn(c, c, 3, 3, 3, generator=g) / float(c * 27) ** 0.5)
    return dict(xa=xa, wa=wa, xb=xb, wb=wb, sc=torch.rand(2 * c, generator=g) + 0.5,
                sh=torch.randn(2 * c, generator=g) * 0.1)


def integer_costvolume_case(seed, c, cout, maxdisp, hw, batch=2):
    g = torch.Generator().manual_seed(seed)
    fl = _ternary(g, (batch, c) + tuple(hw), 0.5)
    fr = _ternary(g, (batch, c) + tuple(hw), 0.5)
    w = _ternary(g, (cout, 2 * c, 3, 3, 3), 0.25)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=g)]
    shift = torch.randint(-4, 5, (cout,), generator=g).float()
    raw = conv_raw(build_cost_volume(fl, fr, maxdisp), w, 3)
    assert_integer_exact(raw, scale, shift, torch.zeros(1))
    return dict(fl=fl, fr=fr, w=w, scale=scale, shift=shift)


def normal_costvolume_case(seed, c, cout, maxdisp, hw, batch=2):
    g = torch.Generator().manual_seed(seed)
    fl = bf(torch.randn((batch, c) + tuple(hw), generator=g))
    fr = bf(torch.randn((batch, c) + tuple(hw), generator=g))
    w = bf(torch.randn(cout, 2 * c, 3, 3, 3, generator=g) / float(2 * c * 27) ** 0.5)
    return dict(fl=fl, fr=fr, w=w, scale=torch.rand(cout, generator=g) + 0.5,
                shift=torch.randn(cout, generator=g) * 0.1)
