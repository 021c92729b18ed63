"""The reference's edge-aware training objective on the device.

``train.py:107-113`` combined_loss = smooth-L1 over the valid pixels + ``edge_loss_w`` *
``gradient_aware_loss2`` (``edge_detection/edge_detection.py:68-74``), whose target the
reference smooths on the host with ``cv2.medianBlur(cv2.medianBlur(t, 5), 5)`` every step.
Here it is three launches (``kernels.median_blur5``, ``edge_loss_sums``, ``edge_loss_grad``)
and a few 0-d tensor ops; nothing is copied to the host and nothing synchronises, so a step
with this loss can be captured in a graph.  Every value returned is a 0-d device tensor.
The loss is differentiable in the prediction only: the target gets no gradient, as in the
reference, where it passes through numpy.

With no valid pixel the direct term and its gradient are 0 (torch's mean over an empty
selection gives NaN; the reference's loop skips such a batch, ``train.py:152``).

``photometric_loss`` is the label-free companion: the right image warped to the left view by
the predicted disparity against the left image (SSIM + L1), a gradient at every in-view
pixel of every batch whatever the target holds.
"""
from __future__ import annotations

import torch

from . import kernels


def smooth_target(target: torch.Tensor) -> torch.Tensor:
    """The reference's ``make_smoother_disp`` on a device tensor: two exact 5x5 median
    passes with a replicated border, [B, H, W] or [H, W] float32."""
    return kernels.median_blur5(target, iterations=2)


make_smoother_disp = smooth_target


class _EdgeAwareLoss(torch.autograd.Function):
    """(predict, target, tsmooth, maxdisp, grad_loss_w) ->
    (combined, direct, edge, epe, n_valid), float32 0-d but n_valid (float64)."""

    @staticmethod
    def forward(ctx, predict, target, tsmooth, maxdisp, grad_loss_w):
        predict = predict.detach()
        sums = kernels.edge_loss_sums(predict, target, tsmooth, maxdisp)
        b, h, w = predict.shape
        n = sums[0]
        has = n > 0
        safe_n = torch.where(has, n, torch.ones_like(n))
        direct = torch.where(has, sums[1] / safe_n, torch.zeros_like(n))
        epe = torch.where(has, sums[2] / safe_n, torch.zeros_like(n))
        edge = sums[3] / float(b * (h - 2) * (w - 2))
        comb = direct + edge * float(grad_loss_w)
        ctx.save_for_backward(predict, target, tsmooth, sums)
        ctx.maxdisp, ctx.w = float(maxdisp), float(grad_loss_w)
        epe, n = epe.float(), n.clone()
        ctx.mark_non_differentiable(epe, n)
        return comb.float(), direct.float(), edge.float(), epe, n

    @staticmethod
    def backward(ctx, g_comb, g_direct, g_edge, _g_epe, _g_n):
        predict, target, tsmooth, sums = ctx.saved_tensors
        scales = torch.stack([g_comb + g_direct, g_comb * ctx.w + g_edge]).float()
        dpred = kernels.edge_loss_grad(predict, target, tsmooth, ctx.maxdisp, sums, scales)
        return dpred, None, None, None, None


def _maps(predict, target):
    if predict.dim() == 4 and predict.shape[1] == 1:
        predict = predict.squeeze(1)
    if target.dim() == 4 and target.shape[1] == 1:
        target = target.squeeze(1)
    kernels._require_cuda(predict, target)
    return predict, target.detach()


def combined_loss(predict: torch.Tensor, target: torch.Tensor, maxdisp: float, grad_loss_w: float = 0.2,
                  return_parts: bool = False):
    """``train.py:107-113`` with the validity mask of ``:116-118`` formed on the device:
    ``direct + grad_loss_w * edge``.  With ``return_parts`` also ``(direct, grad, epe,
    n_valid)``: the two terms, the masked mean absolute error (``train.py:162``) and the
    number of valid pixels, all device scalars."""
    predict, target = _maps(predict, target)
    comb, direct, edge, epe, n = _EdgeAwareLoss.apply(predict, target, smooth_target(target), maxdisp, grad_loss_w)
    return (comb, (direct, edge, epe, n)) if return_parts else comb


def gradient_aware_loss2(output: torch.Tensor, target: torch.Tensor, device=None) -> torch.Tensor:
    """``edge_detection.py:68-74``; ``device`` is accepted for the reference's signature and
    ignored (the tensors' device is used)."""
    output, target = _maps(output, target)
    return _EdgeAwareLoss.apply(output, target, smooth_target(target), float("inf"), 1.0)[2]


def masked_smooth_l1(disp: torch.Tensor, target: torch.Tensor, maxdisp: float) -> torch.Tensor:
    """``F.smooth_l1_loss(disp[mask], target[mask])`` with ``mask = (target < maxdisp) &
    (target > 0.001)`` (``train.py:116-118,157``), without materialising the selection.  The
    edge term is not wanted, so the target stands in for its smoothed form (no median)."""
    disp, target = _maps(disp, target)
    return _EdgeAwareLoss.apply(disp, target, target, maxdisp, 0.0)[1]


class _PhotometricLoss(torch.autograd.Function):
    """(disp, left, right, exclude, alpha) -> (loss, l1, dssim, n_view, n_window), float32
    0-d but the two counts (float64)."""

    @staticmethod
    def forward(ctx, disp, left, right, exclude, alpha):
        disp = disp.detach()
        sums = kernels.photometric_sums(left, right, disp, exclude, alpha)
        n_v, n_w = sums[0], sums[2]
        l1 = sums[1] / n_v.clamp(min=1.0)        # a sum over no pixel is 0: 0 / 1
        dssim = sums[3] / n_w.clamp(min=1.0)
        loss = (1.0 - alpha) * l1 + alpha * dssim
        ctx.save_for_backward(disp, left, right, sums, *(() if exclude is None else (exclude,)))
        ctx.alpha = float(alpha)
        n_v, n_w = n_v.clone(), n_w.clone()
        ctx.mark_non_differentiable(n_v, n_w)
        return loss.float(), l1.float(), dssim.float(), n_v, n_w

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_dssim, _g_nv, _g_nw):
        disp, left, right, sums, *rest = ctx.saved_tensors
        scales = torch.stack([g_loss * (1.0 - ctx.alpha) + g_l1, g_loss * ctx.alpha + g_dssim]).float()
        ddisp = kernels.photometric_grad(left, right, disp, rest[0] if rest else None, sums=sums, scales=scales)
        return ddisp, None, None, None, None


def photometric_loss(left: torch.Tensor, right: torch.Tensor, disp: torch.Tensor, exclude: torch.Tensor = None,
                     alpha: float = 0.85, return_parts: bool = False):
    """Photometric consistency of a disparity map with its image pair, the self-supervised
    signal that needs no target: the right image warped to the left view by ``disp``
    against the left image, ``(1 - alpha) * L1 + alpha * (1 - SSIM) / 2`` over the pixels in
    view (``lea_photometric_f32`` in include/leastereo_hip.h has the definition).  Two
    launches forward, one backward, no host synchronisation; differentiable in ``disp``
    only.  ``left``, ``right``: [B, C, H, W] with C <= 4; ``disp``: [B, H, W] or
    [B, 1, H, W]; ``exclude``: optional [B, H, W] uint8 or bool, non-zero pixels take no part
    (``DisparityLR.state`` as it is).  With ``return_parts`` also ``(l1, dssim, n_view,
    n_window)``, device scalars.  With no pixel in view the loss and its gradient are 0."""
    if disp.dim() == 4 and disp.shape[1] == 1:
        disp = disp.squeeze(1)
    kernels._require_cuda(left, right, disp)
    loss, l1, dssim, n_v, n_w = _PhotometricLoss.apply(disp, left.detach(), right.detach(), exclude, float(alpha))
    return (loss, (l1, dssim, n_v, n_w)) if return_parts else loss
