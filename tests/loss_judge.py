"""The judges of the edge-aware loss tests (CPU only): two independent 5x5 medians with a
replicated border -- OpenCV documents ``medianBlur`` as BORDER_REPLICATE; cv2 itself is not
available to this suite -- and the reference's loss expressions in torch
(``train.py:107-118``, ``edge_detection/edge_detection.py:32-57,68-74``)."""
import numpy as np
import torch
import torch.nn.functional as F


def median5_sort(img: np.ndarray, pad: int = 2, mode: str = "edge") -> np.ndarray:
    """The 13th of the 25 sorted window values over ``img`` padded by ``pad``; the output
    is the padded size less 4 each way (``pad=2``: the size of ``img``)."""
    p = np.pad(img, pad, mode=mode) if pad else img
    h, w = p.shape[0] - 4, p.shape[1] - 4
    win = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)], axis=-1)
    return np.sort(win, axis=-1)[..., 12]


def median5_scipy(img: np.ndarray) -> np.ndarray:
    from scipy import ndimage
    return ndimage.median_filter(img, size=5, mode="nearest")


def median_blur(x: np.ndarray, iterations: int) -> np.ndarray:
    """[B, H, W] -> [B, H, W]: ``iterations`` passes, each replicating ITS input's border."""
    out = []
    for img in x:
        for _ in range(iterations):
            img = median5_sort(img)
        out.append(img)
    return np.stack(out)


def median_twice_of_wide_replicate(x: np.ndarray) -> np.ndarray:
    """The mistaken two-pass form: the input replicated four wide, then two valid medians.
    It differs from ``median_blur(x, 2)`` near the border."""
    return np.stack([median5_sort(median5_sort(img, pad=4), pad=0) for img in x])


SOBEL_X = [[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]]
SOBEL_Y = [[1., 2., 1.], [0., 0., 0.], [-1., -2., -1.]]


def torch_loss(pred, target, tsmooth, maxdisp, w, dtype):
    """The reference's expressions on the CPU in ``dtype``.  Returns direct, edge, combined
    (python floats; direct is None and combined the weighted edge term alone when no pixel
    is valid) and the gradient of combined with respect to pred, [B, H, W] in ``dtype``."""
    o = pred.detach().cpu().to(dtype).clone().requires_grad_()
    t = target.detach().cpu().to(dtype)
    ts = tsmooth.detach().cpu().to(dtype)
    m = (t < maxdisp) & (t > 0.001)
    kx = torch.tensor(SOBEL_X, dtype=dtype).view(1, 1, 3, 3)
    ky = torch.tensor(SOBEL_Y, dtype=dtype).view(1, 1, 3, 3)
    ox, oy = F.conv2d(o.unsqueeze(1), kx), F.conv2d(o.unsqueeze(1), ky)
    tx, ty = F.conv2d(ts.unsqueeze(1), kx), F.conv2d(ts.unsqueeze(1), ky)
    edge = torch.mean(torch.abs(ox) * torch.exp(-torch.abs(tx)) + torch.abs(oy) * torch.exp(-torch.abs(ty)))
    direct = F.smooth_l1_loss(o[m], t[m], reduction="mean") if bool(m.any()) else None
    comb = edge * w if direct is None else direct + edge * w
    comb.backward()
    return (None if direct is None else float(direct.detach())), float(edge.detach()), float(comb.detach()), o.grad
