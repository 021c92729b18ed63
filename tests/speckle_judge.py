"""The speckle filter's definition (lea_disparity_speckle_f32 in include/leastereo_hip.h) in
numpy, in two independent forms, and the input recipes that the CPU and the GPU tests share.

``labels_by_propagation`` iterates label = min(label, connected neighbours' labels) to a fixed
point; ``labels_by_graph`` hands the edge list to scipy's connected_components and re-labels
each component to its smallest index.  Both return (labels, size); ``judge`` derives state
and filtered from them.  Everything is integer-exact except the connectivity test, which is
the kernel's: fabsf(a - b) <= max_diff in float32 (one exactly rounded subtraction).
"""
import numpy as np

LR_SPECKLE = 3


def as_maps(disp, exclude=None):
    d = np.asarray(disp, dtype=np.float32)
    if d.ndim == 2:
        d = d[None]
    assert d.ndim == 3
    e = np.zeros(d.shape, np.uint8) if exclude is None else np.asarray(exclude).astype(np.uint8).reshape(d.shape)
    return d, e


def connectivity(disp, exclude, max_diff):
    """(wall [B, H, W], right [B, H, W-1], down [B, H-1, W]): right[b, y, x] joins (y, x) and (y, x+1)."""
    d, e = as_maps(disp, exclude)
    wall = ~np.isfinite(d) | (e != 0)
    md = np.float32(max_diff)
    with np.errstate(all="ignore"):
        right = (np.abs(d[:, :, :-1] - d[:, :, 1:]) <= md) & ~wall[:, :, :-1] & ~wall[:, :, 1:]
        down = (np.abs(d[:, :-1] - d[:, 1:]) <= md) & ~wall[:, :-1] & ~wall[:, 1:]
    return wall, right, down


def _sizes(labels):
    size = np.zeros(labels.shape, np.int32)
    for b in range(labels.shape[0]):
        lab = labels[b].ravel()
        ok = lab >= 0
        n = np.bincount(lab[ok], minlength=lab.size)
        size[b].ravel()[ok] = n[lab[ok]]
    return size


def labels_by_propagation(disp, exclude, max_diff):
    wall, right, down = connectivity(disp, exclude, max_diff)
    B, H, W = wall.shape
    big = H * W
    lab = np.broadcast_to(np.arange(H * W, dtype=np.int64).reshape(1, H, W), (B, H, W)).copy()
    lab[wall] = big
    sweeps = 0
    while True:
        new = lab.copy()
        new[:, :, :-1] = np.where(right, np.minimum(new[:, :, :-1], new[:, :, 1:]), new[:, :, :-1])
        new[:, :, 1:] = np.where(right, np.minimum(new[:, :, 1:], new[:, :, :-1]), new[:, :, 1:])
        new[:, :-1] = np.where(down, np.minimum(new[:, :-1], new[:, 1:]), new[:, :-1])
        new[:, 1:] = np.where(down, np.minimum(new[:, 1:], new[:, :-1]), new[:, 1:])
        sweeps += 1
        if np.array_equal(new, lab):
            break
        lab = new
    labels = np.where(wall, -1, lab).astype(np.int32)
    labels_by_propagation.sweeps = sweeps
    return labels, _sizes(labels)


def labels_by_graph(disp, exclude, max_diff):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    wall, right, down = connectivity(disp, exclude, max_diff)
    B, H, W = wall.shape
    idx = np.arange(H * W).reshape(H, W)
    labels = np.empty((B, H, W), np.int32)
    for b in range(B):
        src = np.concatenate([idx[:, :-1][right[b]], idx[:-1][down[b]]])
        dst = np.concatenate([idx[:, 1:][right[b]], idx[1:][down[b]]])
        g = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(H * W, H * W))
        _, comp = connected_components(g, directed=False)
        smallest = np.full(comp.max() + 1, H * W, np.int64)
        np.minimum.at(smallest, comp, np.arange(H * W))
        labels[b] = np.where(wall[b], -1, smallest[comp].reshape(H, W))
    return labels, _sizes(labels)


def judge(disp, exclude, max_diff, max_size, fill=0.0, form=labels_by_propagation):
    """dict(labels, size, state, filtered), each of disp's shape, as the header defines them."""
    d, e = as_maps(disp, exclude)
    labels, size = form(d, e, max_diff)
    removed = ((size > 0) & (size <= max_size)) | ~np.isfinite(d)
    state = np.where(e != 0, e, np.where(removed, LR_SPECKLE, 0)).astype(np.uint8)
    filtered = np.where(state != 0, np.float32(fill), d).astype(np.float32)
    shape = np.asarray(disp).shape
    return {"labels": labels.reshape(shape), "size": size.reshape(shape), "state": state.reshape(shape),
            "filtered": filtered.reshape(shape)}


def component_sizes(labels, size):
    """The size of every component, once each."""
    lab, n = np.asarray(labels), np.asarray(size)
    if lab.ndim == 2:
        lab, n = lab[None], n[None]
    idx = np.arange(lab[0].size).reshape(lab.shape[1:])
    return np.concatenate([n[b][lab[b] == idx] for b in range(lab.shape[0])])


# ------------------------------------------------------------------ input recipes

def random_field(shape, seed=0):
    """(disp, exclude) [B, H, W]: random blocks of about H/9 x W/11 pixels with the values
    3 * randint(0, 12) plus uniform(-0.4, 0.4) noise; 8 % of the pixels are salt of +-7, 3 % are
    exclude walls (values 1 and 2) and 1 % are NaN."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    bh, bw = max(1, round(H / 9)), max(1, round(W / 11))
    blocks = 3.0 * rng.integers(0, 12, (B, -(-H // bh), -(-W // bw)))
    d = np.repeat(np.repeat(blocks, bh, axis=1), bw, axis=2)[:, :H, :W]
    d = d + rng.uniform(-0.4, 0.4, shape)
    salt = rng.random(shape) < 0.08
    d = np.where(salt, d + np.where(rng.random(shape) < 0.5, 7.0, -7.0), d)
    d = np.where(rng.random(shape) < 0.01, np.nan, d).astype(np.float32)
    e = np.where(rng.random(shape) < 0.03, rng.integers(1, 3, shape), 0).astype(np.uint8)
    return d, e


def serpentine(H=40, W=90):
    """One corridor that runs along every other row, joined alternately at the right and the
    left end: one component that crosses every tile border (1820 px at 40 x 90); the rows
    between hold a far value, cut by the turns into components of their own."""
    d = np.full((H, W), 100.0, np.float32)
    d[0::2] = 5.0
    for k, y in enumerate(range(1, H, 2)):
        d[y, W - 1 if k % 2 == 0 else 0] = 5.0
    return d


def spiral(H=37, W=70):
    """A rectangular spiral corridor of one pixel, wound inwards with one pixel of wall between
    the turns."""
    d = np.full((H, W), 100.0, np.float32)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    y, x = 0, 0
    d[0, 0] = 5.0
    while right - left >= 2 and bottom - top >= 2:
        for x in range(left, right + 1):
            d[top, x] = 5.0
        for y in range(top, bottom + 1):
            d[y, right] = 5.0
        for x in range(right, left - 1, -1):
            d[bottom, x] = 5.0
        for y in range(bottom, top + 1, -1):
            d[y, left] = 5.0
        d[top + 2, left:left + 3] = 5.0  # step in to the next ring
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return d


def comb(H=40, W=133):
    """A spine along the last row with a one-pixel tooth on every other column: every tooth
    joins the others only at the bottom, the gaps between are components of their own."""
    d = np.full((H, W), 100.0, np.float32)
    d[:, 0::2] = 5.0
    d[H - 1] = 5.0
    return d


def checkerboard(H=35, W=67):
    return (np.indices((H, W)).sum(0) % 2).astype(np.float32)


def constant_pair(H=130, W=70):
    """B = 2, one component per image; image 0's last row equals image 1's first row, so a leak
    between the images of a batch would merge them."""
    return np.full((2, H, W), 7.25, np.float32)


def blob_image(H, W, cy, cx, n, background=10.0, value=50.0):
    """n connected pixels of ``value`` on a constant background, laid boustrophedon over the
    5 x 5 window whose top-left pixel is (cy - 2, cx - 2) clamped into the image: around a tile
    corner at (cy, cx) the blob crosses both seams."""
    assert 1 <= n <= 25
    d = np.full((H, W), background, np.float32)
    y0, x0 = min(max(cy - 2, 0), H - 5), min(max(cx - 2, 0), W - 5)
    for k in range(n):
        r, c = divmod(k, 5)
        d[y0 + r, x0 + (c if r % 2 == 0 else 4 - c)] = value
    return d
