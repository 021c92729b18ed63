"""numpy restatement of lea_disparity_pointcloud_f32 (include/leastereo_hip.h), parameterised by
the dtype of its arithmetic.  float64 is the judge; float32 is the "float32 CPU restatement"
whose own error against the judge sets the bars of tests/test_gpu_pointcloud.py, as
refine_judge.py and photo_judge.py do for their heads.

What is an exact function of the inputs is computed the same way under both dtypes: the
exclude byte, the finiteness and the range of the float32 disparity, and the depth-edge rule
|d_q - d_p| <= normal_max_diff, which the header defines in float32.  Q enters with the float32
values the device reads.  Also the input recipe ``slanted_field`` and its matrix ``recipe_q``."""
import numpy as np

from leastereo_amd.pointcloud import q_matrix


def _as3(a, dtype):
    a = np.asarray(a, dtype)
    return a[None] if a.ndim == 2 else a


def reproject_all(disp, Q, exclude=None, min_disp=0.0, max_disp=np.inf, dtype=np.float64):
    """(P [B, H, W, 3] before masking, valid [B, H, W] bool) of a [B, H, W] float32 map."""
    d32 = _as3(disp, np.float32)
    B, H, W = d32.shape
    q = np.broadcast_to(np.asarray(Q, np.float32).reshape(-1, 4, 4), (B, 4, 4)).astype(dtype)
    x = np.broadcast_to(np.arange(W, dtype=dtype)[None, None, :], (B, H, W))
    y = np.broadcast_to(np.arange(H, dtype=dtype)[None, :, None], (B, H, W))
    d = d32.astype(dtype)
    with np.errstate(all="ignore"):
        h = [((q[:, r, 0, None, None] * x + q[:, r, 1, None, None] * y) + q[:, r, 2, None, None] * d)
             + q[:, r, 3, None, None] for r in range(4)]
        P = np.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], -1).astype(dtype)
        ok = np.isfinite(d32) & (d32 > np.float32(min_disp)) & (d32 <= np.float32(max_disp))
    if exclude is not None:
        ok &= _as3(exclude, np.uint8) == 0
    ok &= np.isfinite(P).all(-1)
    return P, ok


def _shift(a, dy, dx, fill):
    """a[b, y + dy, x + dx], ``fill`` outside the image."""
    out = np.full_like(a, fill)
    H, W = a.shape[1:3]
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[:, yd, xd] = a[:, ys, xs]
    return out


def normals_all(disp, P, valid, normal_max_diff):
    """The normals of every pixel [B, H, W, 3] in P's dtype ((0, 0, 0) where there is none, also at
    invalid pixels), and the diagnostics of the pixels with both differences: ``has`` (bool: a
    normal exists), ``cos`` = |n . P| / |P| and ``rel`` = |dx x dy| / (|dx| |dy|) (NaN elsewhere)."""
    d32 = _as3(disp, np.float32)
    nmd = np.float32(normal_max_diff)
    dt = P.dtype

    def side(dy, dx):
        with np.errstate(all="ignore"):
            near = np.abs(_shift(d32, dy, dx, np.float32(np.nan)) - d32) <= nmd    # float32, as the header says
        return valid & _shift(valid, dy, dx, False) & near, _shift(P, dy, dx, 0)

    def diff(minus, plus):
        (um, Pm), (up, Pp) = minus, plus
        return np.where(up[..., None], Pp, P) - np.where(um[..., None], Pm, P), um | up

    with np.errstate(all="ignore"):
        ddx, hx = diff(side(0, -1), side(0, 1))
        ddy, hy = diff(side(-1, 0), side(1, 0))
        both = hx & hy
        c = np.stack([ddx[..., 1] * ddy[..., 2] - ddx[..., 2] * ddy[..., 1],
                      ddx[..., 2] * ddy[..., 0] - ddx[..., 0] * ddy[..., 2],
                      ddx[..., 0] * ddy[..., 1] - ddx[..., 1] * ddy[..., 0]], -1).astype(dt)
        ln = np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]).astype(dt)
        has = both & (ln > 0) & np.isfinite(ln)
        n = c / ln[..., None]
        dot = (n[..., 0] * P[..., 0] + n[..., 1] * P[..., 1]) + n[..., 2] * P[..., 2]
        n = np.where((dot > 0)[..., None], -n, n)
        n = np.where(has[..., None], n, 0).astype(dt)
        norm = lambda v: np.sqrt((v.astype(np.float64) ** 2).sum(-1))  # noqa: E731
        cos = np.where(has, np.abs(dot) / norm(P), np.nan)
        rel = np.where(both, ln / (norm(ddx) * norm(ddy)), np.nan)
    return n, dict(has=has, both=both, cos=cos, rel=rel)


def judge(disp, Q, image=None, exclude=None, min_disp=0.0, max_disp=np.inf, normals=False, normal_max_diff=1.0,
          capacity=None, dtype=np.float64):
    """Every output of the entry for a [B, H, W] (or [H, W]) map, as a dict: points [B, H, W, 3]
    (``dtype``, NaN where not valid), valid uint8, count int32 [B], and per item b the lists
    xyz[b], rgb[b], index[b], normals[b]: the first min(count[b], capacity) rows.  ``diag``
    holds the diagnostics of ``normals_all``."""
    d32 = _as3(disp, np.float32)
    B, H, W = d32.shape
    capacity = H * W if capacity is None else capacity
    P, ok = reproject_all(d32, Q, exclude, min_disp, max_disp, dtype)
    points = np.where(ok[..., None], P, np.nan).astype(dtype)
    out = dict(points=points, valid=ok.astype(np.uint8), count=ok.reshape(B, -1).sum(1).astype(np.int32),
               xyz=[], rgb=[], index=[], normals=[], diag=None)
    nrm = None
    if normals:
        nrm, out["diag"] = normals_all(d32, P, ok, normal_max_diff)
    img = None if image is None else np.asarray(image, np.uint8).reshape(B, H * W, -1)[..., :3]
    for b in range(B):
        idx = np.flatnonzero(ok[b])[:capacity]                 # row-major order, the first capacity
        out["index"].append(idx.astype(np.int32))
        out["xyz"].append(points[b].reshape(-1, 3)[idx])
        out["rgb"].append(None if img is None else img[b][idx])
        out["normals"].append(None if nrm is None else nrm[b].reshape(-1, 3)[idx])
    return out


# ------------------------------------------------------------------ the input recipe
F, BASELINE = 400.0, 0.25


def recipe_q(H, W, origin=(0, 0)):
    return q_matrix(F, BASELINE, W / 2, H / 2, origin=origin)


def slanted_field(shape, seed):
    """(disp float32, exclude uint8) of ``shape`` = (B, H, W): blocks of about H/5 x W/6 pixels, each
    a plane a + gx x' + gy y' (x', y' from the block's corner) with a in U(8, 60) and gx, gy in
    U(-0.15, 0.15), plus U(-0.02, 0.02) noise; 1 % NaN, 1 % exact zeros, 3 % exclude bytes in 1..3."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    bh, bw = max(1, round(H / 5)), max(1, round(W / 6))
    ny, nx = -(-H // bh), -(-W // bw)
    a = rng.uniform(8, 60, (B, ny, nx))
    gx = rng.uniform(-0.15, 0.15, (B, ny, nx))
    gy = rng.uniform(-0.15, 0.15, (B, ny, nx))
    yy, xx = np.arange(H), np.arange(W)
    by, bx = (yy // bh)[:, None], (xx // bw)[None, :]
    ly, lx = (yy % bh)[:, None], (xx % bw)[None, :]
    d = a[:, by, bx] + gx[:, by, bx] * lx + gy[:, by, bx] * ly + rng.uniform(-0.02, 0.02, shape)
    d = d.astype(np.float32)
    u = rng.random(shape)
    d[u < 0.01] = np.nan
    d[(u >= 0.01) & (u < 0.02)] = 0.0
    e = np.where(rng.random(shape) < 0.03, rng.integers(1, 4, shape), 0).astype(np.uint8)
    return d, e


def recipe_image(shape, seed):
    """A uint8 image [B, H, W, 4] to colour the recipe's points with (the fourth channel is not read)."""
    return np.random.default_rng(seed + 1000).integers(0, 256, tuple(shape) + (4,), dtype=np.uint8)
