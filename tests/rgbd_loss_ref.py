"""fp64 statement of robosimgs_amd.losses.rgbd_loss, the masked RGB-D training loss, in NumPy and in torch.

A helper module of the rgbd_loss tests (not a conftest); SSIM is tests/ssim_ref.py's, unchanged.

Shapes.  render [..., H, W, Cr], Cr in {3, 4}: channels 0..2 colour c, channel 3 (if present) depth d.  target_rgb
[..., H, W, 3] = c*.  target_depth [..., H, W] or None = d*.  mask [..., H, W] or None = m, values in [0, 1], may be soft;
None means m = 1 everywhere.

Masked images.  x = m c where m > 0, else 0;  y = m c* where m > 0, else 0.  A select at m == 0, not a product: a non-finite
render (or target) value under a zero mask contributes exactly 0 to the loss and receives exactly 0 gradient.

Colour term.  (1 - lambda) mean|x - y| + lambda (1 - SSIM(x, y, padding)).  The mean is over all 3 H W images elements
(splatfacto's form: not divided by the mask's area).  SSIM is ssim_ref's, for both paddings, over all of its positions.

Depth term.  w = m where d* is finite and d* > 0, else 0 (a select: a NaN in d* never enters a sum, and neither does d
where w == 0).  D = sum w |d - d*| / sum w over all images together; D = 0 with zero gradient when sum w == 0.
loss = colour + lambda_d D.  lambda_d > 0 needs Cr == 4 and a target_depth; with lambda_d == 0 there is no depth term and
D and sum w are reported as 0.

Gradient, with respect to render only.  Channels 0..2: m times the L1 + D-SSIM gradient evaluated at (x, y), sign(0) = 0.
Channel 3: lambda_d w sign(d - d*) / sum w; with Cr == 4 and lambda_d == 0 it is exactly 0.  (rgbd_loss_torch gives this
through autograd: torch.where routes no gradient to the side it does not select.)

terms = (mean|x - y|, SSIM, D, sum w).
"""
from __future__ import annotations

import numpy as np
import torch

import ssim_ref as S


def _check(render_shape, depth_lambda, target_depth):
    assert render_shape[-1] in (3, 4)
    assert depth_lambda >= 0
    assert depth_lambda == 0 or (render_shape[-1] == 4 and target_depth is not None)


def rgbd_loss_np(render, target_rgb, target_depth=None, mask=None, ssim_lambda=0.2, depth_lambda=0.0, padding="valid"):
    """(loss, (mean|x - y|, SSIM, D, sum w)) as Python floats."""
    render = np.asarray(render, np.float64)
    c, cs = render[..., :3], np.asarray(target_rgb, np.float64)
    _check(render.shape, depth_lambda, target_depth)
    m = np.ones(render.shape[:-1]) if mask is None else np.asarray(mask, np.float64)
    on = (m > 0)[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where(on, m[..., None] * np.where(on, c, 0.0), 0.0)
        y = np.where(on, m[..., None] * np.where(on, cs, 0.0), 0.0)
    l1 = float(np.abs(x - y).mean())
    ssim = S.ssim_np(x, y, padding)
    loss = (1 - ssim_lambda) * l1 + ssim_lambda * (1 - ssim)
    D = sw = 0.0
    if depth_lambda > 0:
        ds = np.asarray(target_depth, np.float64)
        with np.errstate(invalid="ignore"):
            w = np.where(np.isfinite(ds) & (ds > 0), m, 0.0)
        sw = float(w.sum())
        if sw > 0:
            diff = np.where(w > 0, render[..., 3], 0.0) - np.where(w > 0, ds, 0.0)
            D = float((w * np.abs(diff)).sum() / sw)
        loss += depth_lambda * D
    return loss, (l1, ssim, D, sw)


def rgbd_loss_torch(render, target_rgb, target_depth=None, mask=None, ssim_lambda=0.2, depth_lambda=0.0, padding="valid"):
    """The same at render's dtype and device (fp64 for the gradient oracle): (loss, terms), loss differentiable in render."""
    _check(render.shape, depth_lambda, target_depth)
    c, cs = render[..., :3], target_rgb.to(render.dtype)
    m = torch.ones(render.shape[:-1], dtype=render.dtype, device=render.device) if mask is None else mask.to(render.dtype)
    on, zero = (m > 0)[..., None], torch.zeros((), dtype=render.dtype, device=render.device)
    x = m[..., None] * torch.where(on, c, zero)
    y = m[..., None] * torch.where(on, cs, zero)
    l1 = (x - y).abs().mean()
    ssim = S.ssim_torch(x, y, padding)
    loss = (1 - ssim_lambda) * l1 + ssim_lambda * (1 - ssim)
    D = sw = torch.zeros((), dtype=render.dtype, device=render.device)
    if depth_lambda > 0:
        ds = target_depth.to(render.dtype)
        w = torch.where(torch.isfinite(ds) & (ds > 0), m, zero)
        sw = w.sum()
        if float(sw) > 0:
            diff = torch.where(w > 0, render[..., 3], zero) - torch.where(w > 0, ds, zero)
            D = (w * diff.abs()).sum() / sw
        loss = loss + depth_lambda * D
    return loss, (l1.detach(), ssim.detach(), D.detach(), sw.detach())
