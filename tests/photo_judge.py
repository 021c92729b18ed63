"""The judge of the photometric-consistency tests (CPU only): the definition in
include/leastereo_hip.h (lea_photometric_f32) written in torch, run in float64 or float32,
with the gradient from autograd; the closed-form SSIM gradient the kernel uses, in float64;
and the shared test inputs."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

ALPHA, C1, C2 = 0.85, 0.01 ** 2, 0.03 ** 2


def warp(right, disp, dtype):
    """(w [B, C, H, W] in ``dtype``, in_view [B, H, W] bool, slope [B, C, H, W]).  ``disp`` may
    require grad (in ``dtype``); xs is taken from the float32 subtraction and then promoted,
    so every precision agrees on floor and on in_view."""
    b, c, h, w = right.shape
    x = torch.arange(w, dtype=torch.float32).view(1, 1, w)
    d32 = disp.detach().to(torch.float32)
    xs_val = (x - d32).to(dtype)
    in_view = torch.isfinite(d32) & (xs_val >= 0) & (xs_val <= w - 1)
    x0 = torch.where(in_view, torch.clamp(torch.floor(xs_val), max=w - 2), torch.zeros_like(xs_val)).long()
    d = disp.to(dtype)
    xs = xs_val + (d.detach() - d)          # the same value, d xs / d disp = -1
    xs = torch.where(in_view, xs, torch.zeros_like(xs))
    t = (xs - x0.to(dtype)).unsqueeze(1)
    r = right.to(dtype)
    idx = x0.unsqueeze(1).expand(b, c, h, w)
    r0, r1 = torch.gather(r, 3, idx), torch.gather(r, 3, idx + 1)
    wv = torch.where(in_view.unsqueeze(1), r0 + t * (r1 - r0), torch.zeros_like(r0))
    return wv, in_view, r1 - r0


def masks(in_view, exclude):
    """v [B, H, W] and vs [B, H, W] (false on the border) as bool."""
    v = in_view if exclude is None else in_view & (exclude == 0)
    vs = torch.zeros_like(v)
    vs[:, 1:-1, 1:-1] = -F.max_pool2d(-v.double().unsqueeze(1), 3, 1)[:, 0] == 1
    return v, vs


def ssim_map(x, y, c1, c2):
    """[B, C, H-2, W-2], the definition's uncentred form."""
    mx, my = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sx = F.avg_pool2d(x * x, 3, 1) - mx * mx
    sy = F.avg_pool2d(y * y, 3, 1) - my * my
    sxy = F.avg_pool2d(x * y, 3, 1) - mx * my
    return ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx + sy + c2))


def judge(left, right, disp, exclude=None, alpha=ALPHA, c1=C1, c2=C2, dtype=torch.float64, scales=None):
    """Everything the entries give, on the CPU in ``dtype``: a dict of n_view, n_window
    (ints), l1, dssim, loss (python floats; a term whose count is 0 is 0), warped, err,
    l1_map, dssim_map (interior positions, [B, H-2, W-2]), v, vs, and ddisp: the gradient of
    ``scales[0] * l1 + scales[1] * dssim`` (default ``(1 - alpha, alpha)``: the loss)."""
    left, right, disp = left.detach().cpu(), right.detach().cpu(), disp.detach().cpu()
    exclude = None if exclude is None else exclude.detach().cpu()
    g_l, g_s = (1 - alpha, alpha) if scales is None else scales
    d = disp.to(dtype).clone().requires_grad_()
    w, in_view, _ = warp(right, d, dtype)
    v, vs = masks(in_view, exclude)
    lf = left.to(dtype)
    l1_map = (lf - w).abs().mean(1)
    dssim_map = torch.clamp((1 - ssim_map(lf, w, c1, c2)) / 2, 0, 1).mean(1)
    vsi = vs[:, 1:-1, 1:-1]
    n_v, n_w = int(v.sum()), int(vsi.sum())
    l1 = l1_map[v].sum() / n_v if n_v else l1_map.sum() * 0
    dssim = dssim_map[vsi].sum() / n_w if n_w else dssim_map.sum() * 0
    (g_l * l1 + g_s * dssim).backward()
    err = torch.full_like(l1_map, -1.0).detach()
    err[v] = l1_map.detach()[v]
    both = torch.zeros_like(l1_map).detach()
    both[:, 1:-1, 1:-1] = dssim_map.detach()
    err[vs] = ((1 - alpha) * l1_map.detach() + alpha * both)[vs]
    return dict(n_view=n_v, n_window=n_w, l1=float(l1.detach()), dssim=float(dssim.detach()),
                loss=float(((1 - alpha) * l1 + alpha * dssim).detach()), warped=w.detach(), err=err,
                l1_map=l1_map.detach(), dssim_map=dssim_map.detach(), v=v, vs=vs, in_view=in_view, ddisp=d.grad)


def closed_form_ddisp(left, right, disp, exclude=None, c1=C1, c2=C2, scales=(1 - ALPHA, ALPHA)):
    """The gather form of the gradient the kernel uses, in float64 without autograd:
    dS_p/dw_q = (a_p + b_p w_q + c_p L_q) / 9, three box sums of coefficient maps masked by
    vs, times dw/ddisp = -slope; the L1 part by sign(w - L)."""
    dtype = torch.float64
    w, in_view, slope = warp(right.cpu(), disp.detach().cpu(), dtype)
    v, vs = masks(in_view, None if exclude is None else exclude.cpu())
    x, y = left.cpu().to(dtype), w
    c = x.shape[1]
    mx, my = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sx = F.avg_pool2d(x * x, 3, 1) - mx * mx
    sy = F.avg_pool2d(y * y, 3, 1) - my * my
    sxy = F.avg_pool2d(x * y, 3, 1) - mx * my
    n1, n2, d1, d2 = 2 * mx * my + c1, 2 * sxy + c2, mx * mx + my * my + c1, sx + sy + c2
    s = n1 * n2 / (d1 * d2)
    m = vs[:, None, 1:-1, 1:-1].to(dtype)
    ca = (2 * mx * (n2 - n1) / (d1 * d2) - 2 * s * my * (1 / d1 - 1 / d2)) * m
    cb = (-2 * s / d2) * m
    cc = (2 * n1 / (d1 * d2)) * m

    def box(f):  # sum over the windows that hold each pixel: full correlation with ones
        b, ch, h, ww = f.shape
        return F.conv2d(f.reshape(b * ch, 1, h, ww), torch.ones(1, 1, 3, 3, dtype=dtype), padding=2).reshape(
            b, ch, h + 2, ww + 2)

    ds_dw = (box(ca) + box(cb) * y + box(cc) * x) / 9      # d sum_vs S_c / d w_c, per channel
    n_v, n_w = int(v.sum()), int(vs.sum())
    g_l = scales[0] / (n_v * c) if n_v else 0.0
    g_s = scales[1] / (n_w * c) if n_w else 0.0
    dw = g_l * torch.sign(y - x) * v.unsqueeze(1).to(dtype) - 0.5 * g_s * ds_dw
    return -(dw * slope * v.unsqueeze(1).to(dtype)).sum(1)


# ------------------------------------------------------------------ shared inputs

def _seeded(shape, kind):
    return np.random.default_rng([7, *shape, len(kind)])


@functools.lru_cache(None)
def make_case(shape, kind="grid"):
    """left, right [B, C, H, W] N(0, 1); disp [B, H, W]; exclude (uint8 or None), CPU tensors.
    kind "grid": disparities are multiples of 1/64 in [-2, W/2], column 1 rounded to
    integers (xs an integer: pins the floor convention); for the single window (1, 1, 3, 3)
    disp[x] is drawn from [0, x] so that the window exists.  "float": arbitrary float
    disparities in the same range.  "exclude": the grid case with about half of the pixels
    excluded, in random 4 x 4 blocks so that some windows survive.  "smooth": what real pairs
    look like and noise does not -- a smooth scene with an offset (means well above the
    standard deviation in a window, so 1 / d2 is large and the gradient's a + b w + c L
    cancels), left = right shifted by 5 px plus a little noise, float disparities near 5."""
    b, c, h, w = shape
    rng = _seeded(shape, kind)
    if kind == "smooth":
        from scipy import ndimage
        base = ndimage.uniform_filter(rng.standard_normal((b, c, h, w + 5)), size=(1, 1, 7, 7), mode="nearest")
        base = (2.0 + 3.0 * base).astype(np.float32)
        right = np.ascontiguousarray(base[..., 5:])
        left = (base[..., :w] + 0.02 * rng.standard_normal(shape)).astype(np.float32)      # left[x] = right[x - 5]
        disp = (5.0 + 0.3 * rng.standard_normal((b, h, w))).astype(np.float32)
        return torch.from_numpy(left), torch.from_numpy(right), torch.from_numpy(disp), None
    left = rng.standard_normal(shape).astype(np.float32)
    right = rng.standard_normal(shape).astype(np.float32)
    if shape[2:] == (3, 3):
        disp = rng.uniform(0.0, 1.0, (b, h, w)) * np.arange(w)
    else:
        disp = rng.uniform(-2.0, w / 2, (b, h, w))
    if kind != "float":
        disp = np.round(disp * 64) / 64
        disp[:, :, 1] = np.minimum(np.round(disp[:, :, 1]), 1.0 if shape[2:] == (3, 3) else np.inf)
    exclude = None
    if kind == "exclude":
        coarse = rng.random((b, -(-h // 4), -(-w // 4))) < 0.5
        exclude = torch.from_numpy(np.kron(coarse, np.ones((1, 4, 4)))[:, :h, :w].astype(np.uint8))
    return (torch.from_numpy(left), torch.from_numpy(right), torch.from_numpy(disp.astype(np.float32)), exclude)


@functools.lru_cache(None)
def judged(shape, kind="grid", dtype=torch.float64):
    """The judge's result for ``make_case(shape, kind)``, computed once and left unchanged."""
    left, right, disp, exclude = make_case(shape, kind)
    return judge(left, right, disp, exclude, dtype=dtype)
