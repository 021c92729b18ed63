"""Judges of the disparity refinement (lea_disparity_refine_f32 in include/leastereo_hip.h),
in numpy: ``refine64`` is the specification in float64, every line solved by a Thomas sweep;
``refine32`` is the same sweep, in the same order, in float32 -- it exists only to measure
what float32 itself costs on a case (E32), which sets the GPU tests' bar.  ``dense64`` solves
the same systems by assembling them, for the test that pins the judge to the mathematics.
"""
import numpy as np

DEN_MIN = np.float32(1e-30)


def schedule(lam, iterations):
    """lambda_t for t = 1 .. T, in double."""
    T = int(iterations)
    return [1.5 * float(lam) * 4.0 ** (T - t) / (4.0 ** T - 1.0) for t in range(1, T + 1)]


def evidence(disp, conf, exclude, dtype):
    """(c0, f0) [B, H, W] in ``dtype``."""
    disp = np.asarray(disp, dtype=np.float32)
    conf = np.ones_like(disp) if conf is None else np.asarray(conf, dtype=np.float32)
    ok = np.isfinite(disp) & np.isfinite(conf)
    with np.errstate(invalid="ignore"):
        ok &= conf > 0
    if exclude is not None:
        ok &= np.asarray(exclude) == 0
    c0 = np.where(ok, conf, np.float32(0)).astype(dtype)
    f0 = np.where(ok, disp, np.float32(0)).astype(dtype)
    return c0, f0


def weights(guide, sigma, dtype):
    """(wh [B, H, W-1], wv [B, H-1, W]) in ``dtype``: exp(-(max_c |dG|) / sigma)."""
    g = np.asarray(guide, dtype=np.float32).astype(dtype)
    s = dtype(np.float32(sigma))  # the entry takes sigma as float32
    mh = np.abs(g[:, :, :, 1:] - g[:, :, :, :-1]).max(axis=1)
    mv = np.abs(g[:, :, 1:, :] - g[:, :, :-1, :]).max(axis=1)
    return np.exp(-(mh / s)).astype(dtype), np.exp(-(mv / s)).astype(dtype)


def thomas(w, rhs, lam):
    """Solve (I + lam L) u = r along the last axis for every right-hand side in ``rhs``
    (arrays [..., n]); ``w`` [..., n-1] the neighbour weights; everything in w's dtype."""
    dtype = w.dtype.type
    n = rhs[0].shape[-1]
    lam = dtype(lam)
    one = dtype(1)
    zero = np.zeros(rhs[0].shape[:-1], dtype=dtype)
    cp = np.empty(rhs[0].shape, dtype=dtype)
    out = [np.empty(r.shape, dtype=dtype) for r in rhs]
    cprev, prev = zero, [zero for _ in rhs]
    for i in range(n):
        a = -lam * w[..., i - 1] if i > 0 else zero
        c = -lam * w[..., i] if i < n - 1 else zero
        b = one - a - c
        den = b - a * cprev
        cprev = c / den
        cp[..., i] = cprev
        prev = [(r[..., i] - a * p) / den for r, p in zip(rhs, prev)]
        for o, p in zip(out, prev):
            o[..., i] = p
    for o in out:
        for i in range(n - 2, -1, -1):
            o[..., i] = o[..., i] - cp[..., i] * o[..., i + 1]
    return out


def _refine(guide, disp, conf, exclude, lam, sigma, iterations, dtype):
    disp = np.asarray(disp, dtype=np.float32)
    c0, f0 = evidence(disp, conf, exclude, dtype)
    wh, wv = weights(guide, sigma, dtype)
    num, den = c0 * f0, c0
    for lt in schedule(lam, iterations):
        lt = dtype(np.float32(lt))  # the entry casts lambda_t to float32
        num, den = thomas(wh, [num, den], lt)
        num, den = (np.ascontiguousarray(np.swapaxes(t, 1, 2)) for t in (num, den))
        num, den = thomas(np.ascontiguousarray(np.swapaxes(wv, 1, 2)), [num, den], lt)
        num, den = (np.ascontiguousarray(np.swapaxes(t, 1, 2)) for t in (num, den))
    solved = den > dtype(DEN_MIN)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = num / np.where(solved, den, dtype(1))
    fallback = np.where(np.isfinite(disp), disp, np.float32(0))
    refined = np.where(solved, q, fallback.astype(dtype))
    return {"refined": refined, "den": den, "num": num, "solved": solved, "fallback": fallback}


def refine64(guide, disp, conf=None, exclude=None, lam=8000.0, sigma=0.05, iterations=3):
    return _refine(guide, disp, conf, exclude, lam, sigma, iterations, np.float64)


def refine32(guide, disp, conf=None, exclude=None, lam=8000.0, sigma=0.05, iterations=3):
    return _refine(guide, disp, conf, exclude, lam, sigma, iterations, np.float32)


def dense64(guide, disp, conf, exclude, lam, sigma, iterations):
    """num / den by a dense solve of the assembled I + lambda_t L_h, then I + lambda_t L_v."""
    disp = np.asarray(disp, dtype=np.float32)
    c0, f0 = evidence(disp, conf, exclude, np.float64)
    wh, wv = weights(guide, sigma, np.float64)
    B, H, W = disp.shape
    out = np.empty((B, H, W))
    dens = np.empty((B, H, W))
    idx = np.arange(H * W).reshape(H, W)
    for b in range(B):
        def laplacian(p, q, w):
            L = np.zeros((H * W, H * W))
            for i, j, v in zip(p.ravel(), q.ravel(), w.ravel()):
                L[i, i] += v
                L[j, j] += v
                L[i, j] -= v
                L[j, i] -= v
            return L
        Lh = laplacian(idx[:, :-1], idx[:, 1:], wh[b])
        Lv = laplacian(idx[:-1, :], idx[1:, :], wv[b])
        r = np.stack([(c0[b] * f0[b]).ravel(), c0[b].ravel()], 1)
        for lt in schedule(lam, iterations):
            lt = float(np.float32(lt))
            r = np.linalg.solve(np.eye(H * W) + lt * Lh, r)
            r = np.linalg.solve(np.eye(H * W) + lt * Lv, r)
        out[b] = (r[:, 0] / r[:, 1]).reshape(H, W)
        dens[b] = r[:, 1].reshape(H, W)
    return out, dens


def piecewise_guide(rng, B, C, H, W, noise=0.05):
    """A piecewise-constant guide (a few rectangles of random level per channel) plus
    N(0, noise) noise, float32 [B, C, H, W], and the label map [B, H, W] it was drawn from."""
    labels = np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        for k in range(1, 5):
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            y1, x1 = rng.integers(y0, H) + 1, rng.integers(x0, W) + 1
            labels[b, y0:y1, x0:x1] = k
    levels = rng.uniform(-2.0, 2.0, size=(B, C, 5))
    g = np.take_along_axis(levels[:, :, :, None], labels.reshape(B, 1, 1, H * W).repeat(C, 1), axis=2)
    g = g.reshape(B, C, H, W) + rng.normal(0.0, noise, size=(B, C, H, W))
    return g.astype(np.float32), labels


def make_case(shape, seed=0):
    """The GPU accuracy tests' inputs: (guide, disp in 0..90, conf uniform with 30 % zeros)."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    guide, _ = piecewise_guide(rng, B, C, H, W)
    disp = rng.uniform(0.0, 90.0, size=(B, H, W)).astype(np.float32)
    conf = rng.uniform(0.0, 1.0, size=(B, H, W)).astype(np.float32)
    conf[rng.uniform(size=(B, H, W)) < 0.3] = 0.0
    return guide, disp, conf


def bar(got64, want32, peak):
    """max(4 E32, 8 ulp(peak)): E32 the float32 judge's own max error against the float64 one."""
    e32 = float(np.abs(want32.astype(np.float64) - got64).max()) if got64.size else 0.0
    return max(4.0 * e32, 8.0 * float(np.spacing(np.float32(peak)))), e32
