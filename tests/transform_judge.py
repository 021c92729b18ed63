"""CPU judge of the device training transform (lea_train_transform_u8, leastereo_amd/data.py):
a numpy restatement of the reference's loader rules (dataloaders/datasets/common.py:119-131
set_rgb_layers, :43-91 train_transform, :94-116 test_transform) that builds the padded canvas
literally, for shapes the fixture tests/golden/train_transform.npz does not carry.  The
fixture holds the reference's own outputs; tests/test_transform_cpu.py requires every
function here to reproduce it bit for bit, so the judge is itself checked against the
reference.

  * ``standardize``      [8, h, w] float32 planes of one decoded sample (rule 1)
  * ``train_transform``  rules 2-4 with the canvas built as the reference builds it
  * ``test_transform``   the validation geometry, target pad 1000
  * ``apply_params``     what a params row means, for any five ints (window + pad)
  * ``n_valid``          train.py:116-118's count in float32
"""
import numpy as np

PAD_LEFT_DISP = 1000.0


def standardize(left_u8, right_u8, disp_left, disp_right=None):
    """One sample -> [8, h, w] float32: (x - mean) / std per channel over the whole image in
    float64 (population std), rounded once at the store; then the two disparities."""
    h, w = left_u8.shape[:2]
    t = np.zeros([8, h, w], "float32")
    with np.errstate(all="ignore"):
        for i, img in enumerate((left_u8, right_u8)):
            for c in range(3):
                x = img[:, :, c]
                t[3 * i + c] = (x - np.mean(x)) / np.std(x)
    t[6] = disp_left
    if disp_right is not None:
        t[7] = disp_right
    return t


def _canvas(t, hc, wc):
    """The sample at the bottom-right of an hc x wc canvas: 0 everywhere but 1000 in plane 6."""
    _, h, w = t.shape
    c = np.zeros([8, hc, wc], "float32")
    c[6] = PAD_LEFT_DISP
    c[:, hc - h:, wc - w:] = t
    return c


def train_transform(t, ch, cw, use_left=True, left_right=False, shift=0, rng=None):
    """Rules 2-4 on the planes ``t`` of ``standardize``; ``rng.randint`` supplies the draws.
    Returns (left [3,ch,cw], right, target [1,ch,cw], params row)."""
    _, h, w = t.shape
    if h < ch and w > cw:
        raise ValueError("train_transform: empty range")
    if h > ch and w <= cw:
        hc, wc = h + shift, cw + shift
    elif h <= ch and w <= cw:
        hc, wc = ch + shift, cw + shift
    else:
        hc, wc = h, w
    c = _canvas(t, hc, wc)
    py, px = hc - h, wc - w
    if shift > 0:
        sx = rng.randint(0, wc - cw)
        dx = rng.randint(-shift, shift)
        if sx + dx < 0 or sx + dx + cw > wc:
            dx = 0
        sy = rng.randint(0, hc - ch)
        left = c[0:3, sy:sy + ch, sx + dx:sx + dx + cw]
        right = c[3:6, sy:sy + ch, sx:sx + cw]
        target = c[6:7, sy:sy + ch, sx + dx:sx + dx + cw] - np.float32(dx)
        return left, right, target, (sy - py, sx + dx - px, sx - px, dx, 0)
    if h <= ch and w <= cw:
        sx = sy = 0
    else:
        sx = rng.randint(0, wc - cw)
        sy = rng.randint(0, hc - ch)
    c = c[:, sy:sy + ch, sx:sx + cw]
    swap = 0
    if not use_left:
        coin = rng.randint(0, 1)
        swap = 0 if (coin == 0 and left_right) else 1
    if swap:
        return c[3:6], c[0:3], c[7:8], (sy - py, sx - px, sx - px, 0, 1)
    return c[0:3], c[3:6], c[6:7], (sy - py, sx - px, sx - px, 0, 0)


def test_transform(t, ch, cw):
    """common.py:94-116 with use_left: zero-pad top-left up to the crop (target pad 1000), or
    the centre crop."""
    _, h, w = t.shape
    if h <= ch and w <= cw:
        c = _canvas(t, ch, cw)
    else:
        if h < ch or w < cw:
            raise ValueError("test_transform: the image neither fits the crop nor covers it")
        sx, sy = (w - cw) // 2, (h - ch) // 2
        c = t[:, sy:sy + ch, sx:sx + cw]
    return c[0:3], c[3:6], c[6:7]


test_transform.__test__ = False  # a judge, not a test


def _window(plane, y0, x0, ch, cw, pad):
    """plane[y0:y0+ch, x0:x0+cw] with ``pad`` wherever that leaves the plane (python ints:
    any offsets)."""
    h, w = plane.shape
    out = np.full((ch, cw), pad, "float32")
    ya, yb = max(0, -y0), min(ch, h - y0)
    xa, xb = max(0, -x0), min(cw, w - x0)
    if ya < yb and xa < xb:
        out[ya:yb, xa:xb] = plane[y0 + ya:y0 + yb, x0 + xa:x0 + xb]
    return out


def apply_params(t, params, ch, cw, has_right_disp=True):
    """The meaning of one params row on the planes ``t`` -> (left, right, target)."""
    y0, xl, xr, sub, flags = (int(v) for v in params)
    a, b = (t[3:6], t[0:3]) if flags & 1 else (t[0:3], t[3:6])
    left = np.stack([_window(p, y0, xl, ch, cw, 0.0) for p in a])
    right = np.stack([_window(p, y0, xr, ch, cw, 0.0) for p in b])
    if flags & 1:
        disp, pad = (t[7] if has_right_disp else np.zeros_like(t[7])), 0.0
    else:
        disp, pad = t[6], PAD_LEFT_DISP
    target = _window(disp, y0, xl, ch, cw, pad)[None] - np.float32(sub)
    return left, right, target.astype("float32")


def n_valid(target, maxdisp):
    """train.py:116-118 in float32 compares."""
    target = np.asarray(target, "float32")
    return int(np.count_nonzero((target < np.float32(maxdisp)) & (target > np.float32(0.001))))
