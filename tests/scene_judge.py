"""A numpy restatement of whole-scene inference's tile plan, weights and blend, for the tests
to judge the library by.  Plain numpy, nothing from the library.

Axis rule (scene length S, tile length L, guards g0 low / g1 high, ramp r):
  S <= L: one tile at origin S - L.
  else:   smax = L - g0 - g1 - r (>= 1), n = ceil((S - L) / smax) + 1, o_k = k (S - L) // (n - 1).
  The x guards sum to maxdisp + 2 context, the y guards to 2 context.
Weights on one axis, tile coordinate i: lo = o > 0, hi = o + L < S, a = g0 if lo else 0,
b = g1 if hi else 0; w = 0 for i < a or i >= L - b, else
min(i - a + 1 if lo else r, (L - b) - i if hi else r, r).  The 2-D weight is wy * wx.
Left-view maps take the x guards (maxdisp + context, context), the right view's disparity
(context, maxdisp + context); the y guards are (context, context).
Blend, per pixel, over the tiles of positive weight in ascending k = ky * nx + kx: one tile ->
its value copied; several -> num = sum w v, den = sum w, out = num / den, every product, add
and the divide one float32 operation; none -> 0.  A value of weight 0 is never read.
"""
import numpy as np


def axis_origins(S, L, guards, ramp):
    if S <= L:
        return [S - L]
    smax = L - guards - ramp
    if smax < 1:
        raise ValueError("tile too short")
    n = -(-(S - L) // smax) + 1
    return [(k * (S - L)) // (n - 1) for k in range(n)]


def plan(height, width, tile_h, tile_w, maxdisp, context, ramp):
    """(ys, xs)."""
    if not 1 <= ramp <= 256:
        raise ValueError("ramp")
    return (axis_origins(height, tile_h, 2 * context, ramp),
            axis_origins(width, tile_w, maxdisp + 2 * context, ramp))


def guards(maxdisp, context, view):
    gx = (maxdisp + context, context) if view == "left" else (context, maxdisp + context)
    return (context, context), gx


def axis_weight(o, L, S, g0, g1, ramp):
    lo, hi = o > 0, o + L < S
    a, b = (g0 if lo else 0), (g1 if hi else 0)
    w = np.zeros(L, dtype=np.int64)
    for i in range(L):
        if i < a or i >= L - b:
            continue
        w[i] = min(i - a + 1 if lo else ramp, (L - b) - i if hi else ramp, ramp)
    return w


def tile_weights(ys, xs, k, height, width, tile_h, tile_w, maxdisp, context, ramp, view):
    (gy0, gy1), (gx0, gx1) = guards(maxdisp, context, view)
    wy = axis_weight(ys[k // len(xs)], tile_h, height, gy0, gy1, ramp)
    wx = axis_weight(xs[k % len(xs)], tile_w, width, gx0, gx1, ramp)
    return wy[:, None] * wx[None, :]


def blend(tiles, ys, xs, height, width, maxdisp, context, ramp, view):
    """tiles float32 [ny * nx, tile_h, tile_w] -> (out float32 [H, W], cover count int [H, W])."""
    tiles = np.asarray(tiles)
    assert tiles.dtype == np.float32
    _, th, tw = tiles.shape
    n = np.zeros((height, width), dtype=np.int64)
    one = np.zeros((height, width), dtype=np.float32)
    num = np.zeros((height, width), dtype=np.float32)
    den = np.zeros((height, width), dtype=np.float32)
    for k in range(len(ys) * len(xs)):
        oy, ox = ys[k // len(xs)], xs[k % len(xs)]
        w = tile_weights(ys, xs, k, height, width, th, tw, maxdisp, context, ramp, view)
        y0, y1, x0, x1 = max(oy, 0), min(oy + th, height), max(ox, 0), min(ox + tw, width)
        if y0 >= y1 or x0 >= x1:
            continue
        w = w[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        v = tiles[k, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        on = w > 0
        wf = w.astype(np.float32)
        # only where the weight is positive: nothing else of the tile is read
        p = np.zeros(w.shape, dtype=np.float32)
        p[on] = wf[on] * v[on]
        sub = (slice(y0, y1), slice(x0, x1))
        first, more = on & (n[sub] == 0), on & (n[sub] > 0)
        one[sub][first] = v[first]
        num[sub][first] = p[first]
        den[sub][first] = wf[first]
        num[sub][more] = num[sub][more] + p[more]
        den[sub][more] = den[sub][more] + wf[more]
        n[sub][on] += 1
    out = np.zeros((height, width), dtype=np.float32)
    out[n == 1] = one[n == 1]
    out[n > 1] = num[n > 1] / den[n > 1]
    return out, n
