"""numpy judge of the surface model (include/leastereo_hip.h, lea_dsm_splat_f32 /
lea_dsm_resolve_f32), one item at a time.

The scatter is stated twice, independently: ``splat_loop`` walks the rows in Python with integer
keys, ``splat_vec`` is one ``np.maximum.at`` on uint64.  Both use float32 arithmetic in the
header's order (numpy rounds every float32 operation on its own).  ``project64`` /
``splat64`` are the float64 form of the geometry, for the end-to-end error.  The fill passes and
the decoding (``fill_pass``, ``resolve``) have one form only; tests/test_dsm_cpu.py holds it to
hand-made grids.

A plain helper module: no conftest, no pytest setting.
"""
from __future__ import annotations

import collections
import struct

import numpy as np

MAX_COORD = np.float32(2.0 ** 30)
HALF = np.float32(0.5)
FULL = 0xFFFFFFFF


# ---- the key

def ord32(bits):
    """The order-preserving map of float32 bits (uint32 array) to uint32."""
    bits = np.asarray(bits, dtype=np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def unord32(o):
    o = np.asarray(o, dtype=np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)


def _ord_int(z: float) -> int:
    """ord of one float32 from its bytes, with Python integers (the loop form's own route)."""
    b = struct.unpack("<I", struct.pack("<f", z))[0]
    return (~b & FULL) if b >> 31 else (b | 0x80000000)


# ---- the geometry, float32 in the pinned order

def project32(points, G):
    """(u, v, z) float32 [rows] of float32 points [rows, 3] through float32 G [3, 4]."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    G = np.asarray(G, dtype=np.float32).reshape(3, 4)
    with np.errstate(all="ignore"):
        out = [((G[r, 0] * p[:, 0] + G[r, 1] * p[:, 1]) + G[r, 2] * p[:, 2]) + G[r, 3] for r in range(3)]
    assert all(o.dtype == np.float32 for o in out)
    return out


def kept(points, u, v, z):
    """The rows that are not skipped."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ok = np.isfinite(p).all(1) & np.isfinite(u) & np.isfinite(v) & np.isfinite(z)
        ok &= ~(np.abs(u) > MAX_COORD) & ~(np.abs(v) > MAX_COORD)
    return ok


def span(t, radius, n):
    """(first, last, nearest) cell along one axis of float32 coordinates ``t`` (every one inside
    +-2^30), first / last clipped to 0 .. n - 1, nearest not clipped; int64."""
    r = np.float32(radius)
    t = np.asarray(t, dtype=np.float32)
    lo = np.floor((t - r) + HALF).astype(np.int64)
    hi = np.floor((t + r) + HALF).astype(np.int64)
    near = np.floor(t + HALF).astype(np.int64)
    return np.maximum(lo, 0), np.minimum(hi, n - 1), near


def _rows_read(rows, count):
    return rows if count is None else min(max(int(count), 0), rows)


def payloads(rows, colours):
    if colours is None:
        return (FULL - np.arange(rows, dtype=np.int64)).astype(np.uint64)
    c = np.asarray(colours, dtype=np.uint8).reshape(-1, 3).astype(np.uint64)
    return (c[:, 0] << np.uint64(16)) | (c[:, 1] << np.uint64(8)) | c[:, 2]


def splat_vec(points, G, gh, gw, count=None, colours=None, radius=0.0, keys=None, hits=None):
    """One ``add`` on (keys uint64 [gh, gw], hits int32 [gh, gw]); new grids where None.  Returns
    (keys, hits, skipped rows among those read)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = _rows_read(p.shape[0], count)
    keys = np.zeros((gh, gw), np.uint64) if keys is None else keys.copy()
    hits = np.zeros((gh, gw), np.int32) if hits is None else hits.copy()
    pay = payloads(p.shape[0], colours)[:n]
    p = p[:n]
    u, v, z = project32(p, G)
    ok = kept(p, u, v, z)
    idx = np.nonzero(ok)[0]
    c0, c1, nc = span(u[idx], radius, gw)
    r0, r1, nr = span(v[idx], radius, gh)
    key = (ord32(z[idx].view(np.uint32)).astype(np.uint64) << np.uint64(32)) | pay[idx]
    for dy in range(2 * 2 + 1):
        for dx in range(2 * 2 + 1):
            r, c = r0 + dy, c0 + dx
            m = (r <= r1) & (c <= c1)
            np.maximum.at(keys, (r[m], c[m]), key[m])
    m = (nc >= 0) & (nc < gw) & (nr >= 0) & (nr < gh)
    np.add.at(hits, (nr[m], nc[m]), 1)
    return keys, hits, int(n - idx.size)


def splat_loop(points, G, gh, gw, count=None, colours=None, radius=0.0, keys=None, hits=None):
    """``splat_vec`` as a loop over the rows with Python integer keys."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    G = np.asarray(G, dtype=np.float32).reshape(3, 4)
    n = _rows_read(p.shape[0], count)
    grid = [[0] * gw for _ in range(gh)] if keys is None else [[int(k) for k in row] for row in keys]
    cnt = [[0] * gw for _ in range(gh)] if hits is None else [[int(k) for k in row] for row in hits]
    col = None if colours is None else np.asarray(colours, dtype=np.uint8).reshape(-1, 3)
    r = np.float32(radius)
    skipped = 0
    with np.errstate(all="ignore"):
        for row in range(n):
            X, Y, Z = p[row]
            uvz = [((G[k, 0] * X + G[k, 1] * Y) + G[k, 2] * Z) + G[k, 3] for k in range(3)]
            u, v, z = uvz
            if not all(np.isfinite(t) for t in (X, Y, Z, u, v, z)) or abs(u) > MAX_COORD or abs(v) > MAX_COORD:
                skipped += 1
                continue
            x0, x1 = int(np.floor((u - r) + HALF)), int(np.floor((u + r) + HALF))
            y0, y1 = int(np.floor((v - r) + HALF)), int(np.floor((v + r) + HALF))
            pay = FULL - row if col is None else (int(col[row, 0]) << 16) | (int(col[row, 1]) << 8) | int(col[row, 2])
            key = (_ord_int(float(z)) << 32) | pay
            for y in range(max(y0, 0), min(y1, gh - 1) + 1):
                for x in range(max(x0, 0), min(x1, gw - 1) + 1):
                    if key > grid[y][x]:
                        grid[y][x] = key
            nx, ny = int(np.floor(u + HALF)), int(np.floor(v + HALF))
            if 0 <= nx < gw and 0 <= ny < gh:
                cnt[ny][nx] += 1
    return np.array(grid, dtype=np.uint64).reshape(gh, gw), np.array(cnt, dtype=np.int32).reshape(gh, gw), skipped


# ---- resolve

def fill_pass(keys, min_neighbours):
    """One fill pass on uint64 [gh, gw]."""
    gh, gw = keys.shape
    pad = np.zeros((gh + 2, gw + 2), np.uint64)
    pad[1:-1, 1:-1] = keys
    nb = np.stack([pad[1 + dy:1 + dy + gh, 1 + dx:1 + dx + gw] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                   if (dy, dx) != (0, 0)])
    cnt = (nb != 0).sum(0)
    lo = np.where(nb != 0, nb, np.uint64(0xFFFFFFFFFFFFFFFF)).min(0)
    take = (keys == 0) & (cnt >= min_neighbours)
    return np.where(take, lo, keys)


Maps = collections.namedtuple("Maps", "height rgb source state keys")


def resolve(keys, iterations=0, min_neighbours=3, nodata=np.nan):
    """(height f32, rgb u8 [.., 3], source int32, state u8, the keys after the passes)."""
    fin = keys
    for _ in range(iterations):
        fin = fill_pass(fin, min_neighbours)
    hit = fin != 0
    hi = (fin >> np.uint64(32)).astype(np.uint32)
    pay = (fin & np.uint64(FULL)).astype(np.uint32)
    height = np.where(hit, unord32(hi).view(np.float32), np.float32(nodata)).astype(np.float32)
    rgb = np.stack([(pay >> np.uint32(16)) & np.uint32(255), (pay >> np.uint32(8)) & np.uint32(255),
                    pay & np.uint32(255)], -1).astype(np.uint8)
    rgb[~hit] = 0
    source = np.where(hit, (np.uint32(FULL) - pay).view(np.int32), np.int32(-1)).astype(np.int32)
    state = np.where(keys != 0, 0, np.where(hit, 1, 2)).astype(np.uint8)
    return Maps(height, rgb, source, state, fin)


# ---- the float64 form of the geometry

def project64(points, G):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    G = np.asarray(G, dtype=np.float64).reshape(3, 4)
    return [p @ G[r, :3] + G[r, 3] for r in range(3)]


def splat64(points, G, gh, gw, radius=0.0):
    """(height float64 [gh, gw], NaN where empty; source int64, -1 where empty) of finite float64
    points through a float64 G: the highest z wins, among equal z the smallest row."""
    u, v, z = project64(points, G)
    height = np.full((gh, gw), -np.inf)
    source = np.full((gh, gw), -1, np.int64)
    r = float(radius)
    c0 = np.maximum(np.floor((u - r) + 0.5).astype(np.int64), 0)
    c1 = np.minimum(np.floor((u + r) + 0.5).astype(np.int64), gw - 1)
    r0 = np.maximum(np.floor((v - r) + 0.5).astype(np.int64), 0)
    r1 = np.minimum(np.floor((v + r) + 0.5).astype(np.int64), gh - 1)
    for row in np.lexsort((-np.arange(z.size), z)):  # ascending z, descending row: the winner comes last
        if c0[row] <= c1[row] and r0[row] <= r1[row]:
            height[r0[row]:r1[row] + 1, c0[row]:c1[row] + 1] = z[row]
            source[r0[row]:r1[row] + 1, c0[row]:c1[row] + 1] = row
    height[source < 0] = np.nan
    return height, source


# ---- the input recipe, shared by the CPU and the GPU tests

# u = X, v = Y, z = -Z exactly; the negative zeros let Z = +0.0 at X = Y = 0 give the height -0.0
AXIS_G = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-0.0, -0.0, -1, -0.0]], np.float32)


def rotated_g(gh, gw, k=0):
    """A grid turned by 30 degrees about the optical axis around the grid's centre, float32."""
    a = np.deg2rad(30.0 + 7.0 * k)
    c, s = np.cos(a), np.sin(a)
    cx, cy = (gw - 1) / 2, (gh - 1) / 2
    G = np.array([[c, s, 0.01 * k, cx - c * cx - s * cy], [-s, c, 0.0, cy + s * cx - c * cy],
                  [0.0, 0.0, -1.0, 10.0 + k]], np.float64)
    return G.astype(np.float32)


def special_gs():
    """Matrices with values that do not belong in one, [6, 3, 4] float32.  With finite points they
    make u, v or z not finite, or huge, for some rows or for all:
      0  NaN in z's offset: every z is NaN, every row is skipped
      1  +-1e30 beside Z in u and v, denormals beside Y and X: only rows with Z = 0 stay inside 2^30
      2  z = (5e37 Z) + 2e38: every product is finite, the sum overflows from Z = 3 on
      3  z = (3e38 Z) - 3e38: the product overflows from Z = 1.25 on
      4  +inf beside X in u, -inf as v's offset: u is inf (NaN at X = 0), v is -inf
      5  denormal entries and negative zeros alone: every row stays, z = -Z but for the last bits at Z = 0"""
    nan, inf, den = np.nan, np.inf, 1e-42
    g = np.stack([AXIS_G] * 6).astype(np.float32)
    g[0, 2, 3] = nan
    g[1, 0], g[1, 1] = (1, den, 1e30, 0), (-den, 1, -1e30, 0)
    g[2, 2] = (0, 0, 5e37, 2e38)
    g[3, 2] = (0, 0, 3e38, -3e38)
    g[4, 0], g[4, 1] = (inf, 0, 0, 0), (0, 1, 0, -inf)
    g[5, 0], g[5, 2] = (1, den, -den, 0), (-0.0, den, -1, den)
    return g


def skip_reasons(points, G):
    """(rows with a coordinate that is not finite; rows with finite coordinates whose u, v or z is
    not finite; rows with finite u, v, z but |u| or |v| above 2^30): what the kernel's three tests
    answer for, one after the other."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    u, v, z = project32(p, G)
    with np.errstate(all="ignore"):
        bad_p = ~np.isfinite(p).all(1)
        bad_uvz = ~bad_p & ~(np.isfinite(u) & np.isfinite(v) & np.isfinite(z))
        far = ~bad_p & ~bad_uvz & ((np.abs(u) > MAX_COORD) | (np.abs(v) > MAX_COORD))
    return int(bad_p.sum()), int(bad_uvz.sum()), int(far.sum())


def field(seed, rows, gh, gw, colours, planted=True):
    """(points float32 [rows, 3], colours uint8 [rows, 3] or None): 70 % of the rows in the
    middle third of the grid (several to a cell), the rest over the grid and a margin of 3 cells
    around it; heights on a quarter grid, so that equal heights meet.  With ``planted`` (rows >=
    63) the first rows are the special values: not finite and huge coordinates, denormal and
    -0.0 heights (with AXIS_G, z = -Z: Z = +0.0 gives -0.0), u exactly on -0.5, i + 0.5 and
    GW - 0.5, and one point five times with five payloads."""
    rng = np.random.default_rng(seed)
    p = np.empty((rows, 3), np.float32)
    dense = rng.random(rows) < 0.7
    p[:, 0] = np.where(dense, rng.uniform(gw / 3, 2 * gw / 3, rows), rng.uniform(-3, gw + 2, rows))
    p[:, 1] = np.where(dense, rng.uniform(gh / 3, 2 * gh / 3, rows), rng.uniform(-3, gh + 2, rows))
    p[:, 2] = np.round(rng.uniform(0, 4, rows) * 4) / 4
    col = rng.integers(0, 256, (rows, 3), dtype=np.uint8) if colours else None
    if planted and rows >= 63:
        nan, inf, tiny = np.float32(np.nan), np.float32(np.inf), np.float32(1e-42)
        special = [(nan, 1, 1), (1, nan, 1), (1, 1, nan), (inf, 1, 1), (1, -inf, 1), (1, 1, inf), (1, 1, -inf),
                   (1e30, 1, 1), (-1e30, 1, 1), (1, 1e30, 1), (1, 1, 1e30), (1, 1, -1e30), (3e9, 0, 1), (0, -3e9, 1),
                   (0, 0, tiny), (0, 0, -tiny), (0, 0, -0.0), (0, 0, 0.0), (tiny, -tiny, 1),
                   (-0.5, 0, 1), (0.5, 0, 1), (gw - 0.5, 0, 1), (gw - 1.5, 0, 1), (0, -0.5, 1), (0, gh - 0.5, 1),
                   (2.5, 3.5, 1), (np.nextafter(np.float32(-0.5), np.float32(-1)), 0, 1)]
        special += [(gw // 2 + 0.25, gh // 2 + 0.25, 2.0)] * 5  # equal heights, different payloads
        special += [(gw // 2 + 0.25, gh // 2 + 0.25, 12.0)] * 2  # lower: never seen
        sp = np.array(special, np.float32)
        for k in range(0, rows - sp.shape[0] + 1, 512):  # once in every block of rows, as far as they fit
            p[k:k + sp.shape[0]] = sp
    return p, col


Case = collections.namedtuple("Case", "name gh gw points G count colours radius conditions")


def cases():
    """The fields of the GPU tests, batched: points [B, rows, 3], G [B, 3, 4] or [3, 4], count
    int32 [B] or None, colours [B, rows, 3] or None."""
    out = []

    def one(name, seed, rows, gh, gw, colours, radius, G, conditions=False):
        p, c = field(seed, rows, gh, gw, colours)
        out.append(Case(name, gh, gw, p[None], G, None, None if c is None else c[None], radius, conditions))

    one("1x1_r1", 1, 1, 1, 1, False, 0.0, AXIS_G)
    out[-1].points[0, 0] = (0.25, -0.25, 3.0)
    one("1x7_r63", 2, 63, 1, 7, True, 0.5, AXIS_G)
    one("7x1_r64", 3, 64, 7, 1, False, 2.0, AXIS_G)
    one("65x63_r65", 4, 65, 65, 63, True, 0.5, rotated_g(65, 63))
    one("65x63_r1025_r0", 5, 1025, 65, 63, False, 0.0, AXIS_G, True)
    one("65x63_r1025_rgb", 6, 1025, 65, 63, True, 2.0, rotated_g(65, 63, 1), True)
    one("130x70_r1025", 7, 1025, 130, 70, False, 2.0, AXIS_G, True)
    one("130x70_r1025_rot", 8, 1025, 130, 70, True, 0.5, rotated_g(130, 70, 2))
    # the batch: another G per item; counts 0, below rows (random bits beyond), above rows, rows
    ps, cs = zip(*(field(20 + b, 1500, 65, 63, True) for b in range(4)))
    pts = np.stack(ps)
    junk = np.random.default_rng(99).integers(0, 2 ** 32, (800, 3), dtype=np.uint64).astype(np.uint32)
    pts[1, 700:] = junk.view(np.float32)
    G = np.stack([AXIS_G, AXIS_G, rotated_g(65, 63, 1), rotated_g(65, 63, 3)])
    out.append(Case("65x63_b4_r1500", 65, 63, pts, G, np.array([0, 700, 1700, 1500], np.int32), np.stack(cs), 0.5,
                    True))
    # values that do not belong in a G, an item each; no colours, so that the winner's row is compared too
    ps = [field(40 + b, 1025, 65, 63, False)[0] for b in range(6)]
    out.append(Case("65x63_b6_special_g", 65, 63, np.stack(ps), special_gs(), None, None, 0.5, False))
    # contention: 4096 rows in one cell
    rng = np.random.default_rng(11)
    p = np.empty((4096, 3), np.float32)
    p[:, 0] = 30 + rng.uniform(-0.4, 0.4, 4096)
    p[:, 1] = 31 + rng.uniform(-0.4, 0.4, 4096)
    p[:, 2] = np.round(rng.uniform(0, 2, 4096) * 8) / 8
    out.append(Case("one_cell_4096", 65, 63, p[None], AXIS_G, None, None, 0.0, False))
    out.append(Case("one_cell_4096_rgb", 65, 63, p[None], AXIS_G, None,
                    rng.integers(0, 256, (1, 4096, 3), dtype=np.uint8), 0.0, False))
    return out


FILL = dict(iterations=2, min_neighbours=3)


def judge_case(case, splat=splat_vec):
    """Per item: (keys, hits, skipped, Maps after FILL) of a case, and the rows read."""
    B = case.points.shape[0]
    res = []
    for b in range(B):
        G = case.G if case.G.ndim == 2 else case.G[b]
        cnt = None if case.count is None else case.count[b]
        col = None if case.colours is None else case.colours[b]
        keys, hits, skipped = splat(case.points[b], G, case.gh, case.gw, cnt, col, case.radius)
        res.append((keys, hits, skipped, resolve(keys, **FILL), _rows_read(case.points.shape[1], cnt)))
    return res


def cover_counts(case):
    """How many of the rows read cover each cell, [B, gh, gw] (a third, plain statement of the spans)."""
    B = case.points.shape[0]
    out = np.zeros((B, case.gh, case.gw), np.int64)
    for b in range(B):
        G = case.G if case.G.ndim == 2 else case.G[b]
        n = _rows_read(case.points.shape[1], None if case.count is None else case.count[b])
        p = case.points[b, :n]
        u, v, z = project32(p, G)
        idx = np.nonzero(kept(p, u, v, z))[0]
        c0, c1, _ = span(u[idx], case.radius, case.gw)
        r0, r1, _ = span(v[idx], case.radius, case.gh)
        for a, bb, c, d in zip(r0, r1, c0, c1):
            if a <= bb and c <= d:
                out[b, a:bb + 1, c:d + 1] += 1
    return out


# ---- a layered scene by construction: a ground plane and a box under a nadir rig

SCENE = dict(h=48, w=64, focal=64.0, baseline=0.5, cx=32.0, cy=24.0, z_ground=8.0, z_roof=6.0, box=(16, 32, 20, 44),
             cell=0.125, radius=0.5)


def layered_scene():
    """(disp float32 [2, h, w], Q float64, G64 float64 [3, 4], gh, gw, roof cells): item 0 sees the
    box on the ground, d = f B / Z; item 1 is the bare ground, as a view from elsewhere would
    see it under the box, so that the roof and the ground meet in the roof's cells.  The grid has
    the ground's sample distance as its cell and is shifted by 0.3 cells against the pixel grid:
    no point of the scene lands within 0.05 cells of the edge of a footprint, so the float32
    and the float64 geometry assign nearly every cell the same row.  ``roof cells`` is the
    (rows, columns) slice pair of the cells that lie well inside the roof."""
    from leastereo_amd.dsm import grid_matrix64
    from leastereo_amd.pointcloud import q_matrix
    s = SCENE
    fb = s["focal"] * s["baseline"]
    d = np.full((2, s["h"], s["w"]), fb / s["z_ground"], np.float32)
    y0, y1, x0, x1 = s["box"]
    d[0, y0:y1, x0:x1] = np.float32(fb / s["z_roof"])
    Q = q_matrix(s["focal"], s["baseline"], s["cx"], s["cy"])
    c = s["cell"]
    G64 = grid_matrix64((-(s["cx"] + 0.3) * c, -(s["cy"] + 0.3) * c, 0.0), c)
    gh, gw = s["h"] + 1, s["w"] + 1
    k = s["z_roof"] / s["z_ground"]  # a roof pixel x lands on column k (x - cx) + cx + 0.3
    cols = slice(int(np.ceil(k * (x0 - s["cx"]) + s["cx"] + 0.3)) + 1, int(k * (x1 - 1 - s["cx"]) + s["cx"] + 0.3))
    rows = slice(int(np.ceil(k * (y0 - s["cy"]) + s["cy"] + 0.3)) + 1, int(k * (y1 - 1 - s["cy"]) + s["cy"] + 0.3))
    return d, Q, G64, gh, gw, (rows, cols)


def scene_judges(points32, disp, Q, G64, gh, gw):
    """The float32 judge on the float32 points [rows, 3] given (rows in the order item 0, item 1) and the
    float64 judge on the float64 points of the same pixels: (Maps, height64, source64, agree) with
    ``agree`` the cells to which both assign the same row."""
    from tests import pointcloud_judge as pj
    p64 = pj.reproject_all(disp, Q, dtype=np.float64)[0].reshape(-1, 3)
    keys = splat_vec(points32, G64.astype(np.float32), gh, gw, radius=SCENE["radius"])[0]
    m = resolve(keys)
    h64, s64 = splat64(p64, np.asarray(G64.astype(np.float32), np.float64), gh, gw, SCENE["radius"])
    return m, h64, s64, (m.source >= 0) & (m.source == s64)
