"""float32 judge of ``lea_forward_warp_f32``: the rules of include/leastereo_hip.h restated in
numpy, row by row, every operation one float32 operation (numpy's float32 scalars and arrays
round each operation on its own and never fuse two).

Two independent forms of the same rules:
  ``form="scatter"``  every source column offers its point and its segment's targets, the way a
                      rasteriser walks primitives; the fill is two carry scans
  ``form="gather"``   brute force: for every target u every source column is tried, and every
                      hole searches its row outwards
tests/test_warp_cpu.py holds the two equal; the GPU tests compare the kernel with the first.

Also here: the fields the tests warp (``scene_field``), the two fractions every GPU case must
reach (``hole_fraction``, ``occluded_fraction``), and the layered scene with a right view known
by construction (``layered_scene``).
"""
import numpy as np

F = np.float32
ONE = F(1)


def _lerp(a, v0, v1):
    return ((ONE - a) * v0) + (a * v1)


def _row_setup(d, e, s, max_diff, max_stretch):
    """t, ok per column and which segments exist (all arrays, float32 arithmetic)."""
    W = d.shape[0]
    with np.errstate(all="ignore"):
        t = np.arange(W, dtype=F) - (F(s) * d)
        ok = np.isfinite(d) & np.isfinite(t)
        if e is not None:
            ok &= e == 0
        seg = np.zeros(W, bool)
        if W > 1:
            dd = np.abs(d[1:] - d[:-1])
            den = t[1:] - t[:-1]
            seg[:-1] = ok[:-1] & ok[1:] & (dd <= F(max_diff)) & (den > 0) & (den <= F(max_stretch))
    return t, ok, seg


def _better(z, x, kind, best):
    """does candidate (z, x, kind) beat best = (z, x, kind, a) or None?"""
    if best is None:
        return True
    bz, bx, bk = best[0], best[1], best[2]
    if z != bz:  # as numbers: -0 == +0
        return z > bz
    return (x, kind) > (bx, bk)


def _winners_scatter(d, t, ok, seg):
    W = d.shape[0]
    best = [None] * W
    wmax = F(W - 1)
    with np.errstate(all="ignore"):
        for x in range(W):
            if not ok[x]:
                continue
            up = np.rint(t[x])
            if F(0) <= up <= wmax and _better(d[x], x, 0, best[int(up)]):
                best[int(up)] = (d[x], x, 0, F(0))
            if not seg[x]:
                continue
            t0, t1 = t[x], t[x + 1]
            den = t1 - t0
            lo, hi = max(np.ceil(t0), F(0)), min(np.floor(t1), wmax)
            if not lo <= hi:
                continue
            for u in range(int(lo), int(hi) + 1):
                a = (F(u) - t0) / den
                z = _lerp(a, d[x], d[x + 1])
                if _better(z, x, 1, best[u]):
                    best[u] = (z, x, 1, a)
    return best


def _winners_gather(d, t, ok, seg):
    W = d.shape[0]
    best = [None] * W
    with np.errstate(all="ignore"):
        for u in range(W):
            fu = F(u)
            for x in range(W):
                if not ok[x]:
                    continue
                if np.rint(t[x]) == fu and _better(d[x], x, 0, best[u]):
                    best[u] = (d[x], x, 0, F(0))
                if seg[x] and t[x] <= fu <= t[x + 1]:
                    a = (fu - t[x]) / (t[x + 1] - t[x])
                    z = _lerp(a, d[x], d[x + 1])
                    if _better(z, x, 1, best[u]):
                        best[u] = (z, x, 1, a)
    return best


def _fill_from_scatter(hit):
    """per target the index of the hit it copies, -1 for none: two carry scans."""
    W = len(hit)
    left = np.full(W, -1)
    right = np.full(W, -1)
    c = -1
    for u in range(W):
        if hit[u]:
            c = u
        left[u] = c
    c = -1
    for u in range(W - 1, -1, -1):
        if hit[u]:
            c = u
        right[u] = c
    return left, right


def _fill_from_gather(hit):
    W = len(hit)
    left = np.full(W, -1)
    right = np.full(W, -1)
    for u in range(W):
        for v in range(u, -1, -1):
            if hit[v]:
                left[u] = v
                break
        for v in range(u, W):
            if hit[v]:
                right[u] = v
                break
    return left, right


def warp_row(img, d, e, s, max_diff, max_stretch, fill, fill_value, form="scatter"):
    """One row.  img [C, W], d [W] float32, e [W] bytes or None -> warped [C, W], zview, state, source."""
    C, W = img.shape
    t, ok, seg = _row_setup(d, e, s, max_diff, max_stretch)
    best = (_winners_scatter if form == "scatter" else _winners_gather)(d, t, ok, seg)
    warped = np.full((C, W), F(fill_value), F)
    zview = np.full(W, np.nan, F)
    state = np.ones(W, np.uint8)
    source = np.full(W, -1, F)
    with np.errstate(all="ignore"):
        for u, bst in enumerate(best):
            if bst is None:
                continue
            z, x, kind, a = bst
            state[u] = 0
            zview[u] = z
            source[u] = F(x) + a
            for c in range(C):
                warped[c, u] = _lerp(a, img[c, x], img[c, x + 1]) if kind else img[c, x]
    if fill:
        hit = state == 0
        left, right = (_fill_from_scatter if form == "scatter" else _fill_from_gather)(hit)
        for u in range(W):
            if hit[u]:
                continue
            l, r = left[u], right[u]
            if l < 0 and r < 0:
                continue
            p = l
            if l < 0 or (r >= 0 and zview[r] < zview[l]):
                p = r
            warped[:, u] = warped[:, p]
            zview[u] = zview[p]
        # the copies above read hits only: left / right index hits, never holes
    return warped, zview, state, source


def forward_warp_judge(image, disp, scales, exclude=None, max_diff=1.0, max_stretch=4.0, fill=1, fill_value=0.0,
                       form="scatter"):
    """image [B, C, H, W], disp [B, H, W] float32, scales [B], exclude [B, H, W] bytes or None ->
    dict(warped, zview, state, source)."""
    image, disp = np.asarray(image, F), np.asarray(disp, F)
    B, C, H, W = image.shape
    out = dict(warped=np.empty((B, C, H, W), F), zview=np.empty((B, H, W), F), state=np.empty((B, H, W), np.uint8),
               source=np.empty((B, H, W), F))
    for b in range(B):
        for y in range(H):
            e = None if exclude is None else np.asarray(exclude[b, y])
            w, z, st, so = warp_row(image[b, :, y], disp[b, y], e, F(scales[b]), max_diff, max_stretch, fill,
                                    fill_value, form)
            out["warped"][b, :, y], out["zview"][b, y], out["state"][b, y], out["source"][b, y] = w, z, st, so
    return out


def same_bits(a, b):
    """equal bit for bit, NaN payloads and the sign of zero included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    return bool(np.array_equal(a, b))


# ---- fields

def scene_field(B, H, W, dmax, seed=0):
    """A sloped background with three raised, slightly slanted boxes and 0.05 px noise: disp
    [B, H, W] in about 0.1 dmax .. dmax.  The boxes stand 0.35 .. 0.6 dmax above the background,
    so a warp at a non-zero scale opens holes beside them and hides background behind them."""
    rng = np.random.default_rng(seed)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    out = np.empty((B, H, W), F)
    for b in range(B):
        d = dmax * (0.1 + 0.25 * x / max(W - 1, 1) + 0.05 * y / max(H - 1, 1)) + 0 * y
        for k in range(3):
            w = max(2, int(W * rng.uniform(0.08, 0.2)))
            x0 = int(rng.uniform(0.05 + 0.3 * k, 0.1 + 0.3 * k) * W)
            h0 = int(rng.integers(0, max(H // 3, 1)))
            h1 = H - int(rng.integers(0, max(H // 3, 1)))
            top = dmax * rng.uniform(0.45, 0.7)
            slant = rng.uniform(-0.04, 0.04)
            box = top + slant * (x - x0) + 0 * y
            m = (x >= x0) & (x < x0 + w) & (y >= h0) & (y < h1)
            d = np.where(m, box, d)
        d = d + rng.normal(0.0, 0.05, (H, W))
        out[b] = d.astype(F)
    return out


def texture(B, C, H, W, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, (B, C, H, W)).astype(F)


# for threshold_rows: den = 1.5 at 1, exactly max_stretch = 2 at 2, just above it at the next float
THRESHOLD_SCALES = [1.0, 2.0, float(np.nextafter(F(2), F(3)))]


def threshold_rows():
    """Rows whose neighbours differ by exactly max_diff = 0.5 (connected) and by the next float
    above it (torn), and whose spans are exactly max_stretch = 2 (kept) and just above (torn), at
    s = 1 where den = 1 - (d1 - d0)."""
    up = np.nextafter(F(3.5), F(4))  # 3 + (0.5 + 2^-22), exactly
    rows = [
        [3, 3.5, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3],            # |dd| = 0.5: connected
        [3, up, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3],             # just above: torn
        [4, 4, 4, 3.5, 3, 2.5, 2, 2, 2, 2, 2, 2],          # falling by 0.5: den = 1.5, and 2 at s = 2
        [8, 8, 8, 8, 7.5, 7, 6.5, 6, 6, 6, 6, 6],          # the same further in
    ]
    d = np.array(rows, F)[None]
    im = texture(1, 1, d.shape[1], d.shape[2], seed=9)
    return d, im


def hole_fraction(judged):
    return float((judged["state"] != 0).mean())


def occluded_fraction(judged, disp, scales):
    """The share of source pixels hidden behind another surface: the pixel's own target
    u = rintf(x - s d) lies in the view, and what is seen there comes from more than one column
    away.  (A visible pixel is seen through its own point or one of its two segments, whose
    source lies within one column of it.)"""
    B, H, W = disp.shape
    x = np.arange(W, dtype=F)
    n = 0
    with np.errstate(all="ignore"):
        for b in range(B):
            t = x[None, :] - (F(scales[b]) * disp[b])
            up = np.rint(t)
            inview = np.isfinite(disp[b]) & (up >= 0) & (up <= W - 1)
            ui = np.where(inview, up, 0).astype(np.int64)
            src = np.take_along_axis(judged["source"][b], ui, axis=1)
            n += int((inview & (np.abs(src - x[None, :]) > 1)).sum())
    return n / float(B * H * W)


def layered_scene(H=6, W=96, seed=3):
    """Fronto-parallel layers of integer disparity over a background, with a texture per layer
    defined in the right view, so both views and both disparities are known by construction:
    dict(left [1, 3, H, W], right, disp_left [1, H, W], disp_right, right_from_left): a layer of
    disparity d covering right columns u0 .. u1 covers left columns u0 + d .. u1 + d; each view
    shows the nearest covering layer.  ``right_from_left`` marks the right pixels whose surface
    is also seen in the left view (the others must be holes of the s = 1 warp)."""
    rng = np.random.default_rng(seed)
    # (d, u0, u1) in the right view; no two raised layers overlap in either view, and background
    # is seen between the hole band of one and the next
    layers = [(3, 0, W - 1), (9, 14, 30), (14, 40, 52), (6, 68, 84)]
    tex = rng.uniform(-2.0, 2.0, (len(layers), 3, H, 2 * W)).astype(F)
    left = np.zeros((1, 3, H, W), F)
    right = np.zeros((1, 3, H, W), F)
    dl = np.zeros((1, H, W), F)
    dr = np.zeros((1, H, W), F)
    lk = np.zeros(W, int)
    rk = np.zeros(W, int)
    for col in range(W):
        # nearest layer covering this column in each view
        lk[col] = max((k for k, (d, u0, u1) in enumerate(layers) if (u0 <= col - d <= u1) or k == 0),
                      key=lambda k: layers[k][0])
        rk[col] = max((k for k, (d, u0, u1) in enumerate(layers) if u0 <= col <= u1), key=lambda k: layers[k][0])
        dL, dR = layers[lk[col]][0], layers[rk[col]][0]
        dl[0, :, col], dr[0, :, col] = dL, dR
        left[0, :, :, col] = tex[lk[col], :, :, col - dL + W // 2]
        right[0, :, :, col] = tex[rk[col], :, :, col + W // 2]
    seen = np.zeros(W, bool)
    for u in range(W):
        xs = u + layers[rk[u]][0]
        seen[u] = xs <= W - 1 and lk[xs] == rk[u]
    return dict(left=left, right=right, disp_left=dl, disp_right=dr, right_from_left=seen)
