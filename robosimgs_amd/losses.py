"""Loss terms of the training step as fused HIP kernels.  `l1_loss(render, target)` is
`(render - target).abs().mean()` with its gradient.  Where the render wants a gradient the forward is ONE streaming
launch that also leaves sign(render - target) / n (mgs_l1_loss_fwd_grad) and the backward a launch that does nothing
for the usual grad_output of 1 (mgs_l1_loss_bwd_scale); without a gradient, mgs_l1_loss_fwd alone.  Instead of six
elementwise / reduction kernels of eager PyTorch; bit-reproducible.

`l1_ssim_loss(render, target)` is splatfacto's photometric loss (1 - lambda) L1 + lambda (1 - SSIM) and `ssim(render,
target)` the SSIM term alone, both over images laid out [..., H, W, ch] as the renderer returns them.  The same pattern:
one pass over render and target that leaves the loss's per-tile sums and the complete gradient for a cotangent of 1
(loss.hip: ssim_kernel), one block that adds the sums up; the backward launches nothing for `unit_gradient(loss)`.

SSIM is pytorch_msssim's `SSIM(data_range=1.0, size_average=True)`: an 11-tap Gaussian window of sigma 1.5, applied
separably per channel, C1 = 0.01^2, C2 = 0.03^2, the mean over positions, channels and leading dimensions.
padding="valid" (default; pytorch_msssim and gsplat's simple_trainer) takes S where the whole window lies inside the image,
(H - 10) x (W - 10) positions, and raises ValueError below 11 pixels (pytorch_msssim instead skips filtering along such an
axis, with a warning); padding="same" (the original 3DGS code's `ssim()`) zero-pads by 5 pixels and takes S at every pixel.

`rgbd_loss(render, target_rgb, target_depth, mask)` is that loss on the RGB+ED frame as the renderer leaves it: the mask
applied to both images before either term, an L1 depth term on the fourth channel, the four-channel frame read in place
and its complete cotangent written in the same launches (loss.hip: ssim_kernel<., true>)."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import check, ptr, require_device, sized_call, stream_handle
from .ops import _f32c


_ONES: dict = {}


def unit_gradient(loss: torch.Tensor) -> torch.Tensor:
    """A cached scalar 1.0 on `loss`'s device for `loss.backward(gradient=unit_gradient(loss))`: autograd then needs no
    `ones_like` fill launch, and `l1_loss`'s backward, handed this very tensor, knows the cotangent is 1 without reading it
    and skips its scale launch -- two launches less per training step (`Trainer.step` does this).  Never written to."""
    key = (loss.device.type, loss.device.index)
    one = _ONES.get(key)
    if one is None:
        one = _ONES[key] = torch.ones((), dtype=torch.float32, device=loss.device)
    return one


def _is_unit(g: torch.Tensor) -> bool:
    """g is unit_gradient's tensor: the cotangent is 1 (known without reading it)."""
    one = _ONES.get((g.device.type, g.device.index))
    return one is not None and g.data_ptr() == one.data_ptr()


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        n = a.numel()
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        if not ctx.needs_input_grad[0]:
            sized_call(_lib.lib().mgs_l1_loss_fwd, [n, ptr(a), ptr(b), ptr(loss)], a.device, cached=False, trailing=(None,))
            return loss
        v_a = torch.empty_like(a)
        sized_call(_lib.lib().mgs_l1_loss_fwd_grad, [n, ptr(a), ptr(b), ptr(loss), ptr(v_a)], a.device, cached=False,
                   trailing=(None,))
        ctx.save_for_backward(a, b)
        ctx.v_a = v_a
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        g = _f32c(v_loss)
        v_a, ctx.v_a = ctx.v_a, None
        if v_a is not None:
            if not _is_unit(g):          # (unit_gradient's tensor: the cotangent is 1, nothing to scale)
                check(_lib.lib().mgs_l1_loss_bwd_scale(v_a.numel(), ptr(g), ptr(v_a), stream_handle()), "mgs_l1_loss_bwd_scale")
            return v_a, None
        # a second backward through a retained graph: autograd owns the first buffer by now
        a, b = ctx.saved_tensors
        v_a = torch.empty_like(a)
        check(_lib.lib().mgs_l1_loss_bwd(a.numel(), ptr(a), ptr(b), ptr(g), ptr(v_a), stream_handle(), None), "mgs_l1_loss_bwd")
        return v_a, None


def l1_loss(render: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean |render - target| (scalar tensor); gradient flows to `render` only."""
    if render.shape != target.shape:
        raise ValueError(f"shape mismatch {tuple(render.shape)} vs {tuple(target.shape)}")
    require_device(render, target)
    a, b = _f32c(render), _f32c(target.detach())
    if a.data_ptr() % 16:            # a contiguous view at an odd offset: the kernels load float4
        a = a.clone()
    if b.data_ptr() % 16:
        b = b.clone()
    return _L1.apply(a, b)


class _L1SSIM(torch.autograd.Function):
    """_L1 under an mgs_image_loss descriptor: the forward leaves the gradient for a cotangent of 1 (mgs_l1_loss_fwd_grad),
    any other cotangent scales it once, a second backward recomputes it (mgs_l1_loss_bwd)."""

    @staticmethod
    def forward(ctx, a, b, desc):
        n = a.numel()
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        if not ctx.needs_input_grad[0]:
            sized_call(_lib.lib().mgs_l1_loss_fwd, [n, ptr(a), ptr(b), ptr(loss)], a.device, cached=False,
                       trailing=(ctypes.byref(desc),))
            return loss
        v_a = torch.empty_like(a)
        sized_call(_lib.lib().mgs_l1_loss_fwd_grad, [n, ptr(a), ptr(b), ptr(loss), ptr(v_a)], a.device, cached=False,
                   trailing=(ctypes.byref(desc),))
        ctx.save_for_backward(a, b)
        ctx.v_a, ctx.desc = v_a, desc
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        g = _f32c(v_loss)
        v_a, ctx.v_a = ctx.v_a, None
        if v_a is not None:
            if not _is_unit(g):
                v_a.mul_(g)
            return v_a, None, None
        a, b = ctx.saved_tensors
        v_a = torch.empty_like(a)
        check(_lib.lib().mgs_l1_loss_bwd(a.numel(), ptr(a), ptr(b), ptr(g), ptr(v_a), stream_handle(), ctypes.byref(ctx.desc)),
              "mgs_l1_loss_bwd")
        return v_a, None, None


_PADDING = {"valid": _lib.MGS_SSIM_VALID, "same": _lib.MGS_SSIM_SAME}


def _image_loss(shape, ssim_lambda: float, padding: str) -> "_lib.ImageLoss":
    if padding not in _PADDING:
        raise ValueError(f"padding must be 'valid' or 'same', got {padding!r}")
    if len(shape) < 3:
        raise ValueError(f"expected images [..., H, W, ch], got shape {tuple(shape)}")
    h, w, ch = (int(v) for v in shape[-3:])
    images = math.prod(int(v) for v in shape[:-3])
    if not 1 <= ch <= 4:
        raise ValueError(f"ch = {ch}: 1 to 4 channels (the last dimension)")
    if images < 1 or h < 1 or w < 1:
        raise ValueError(f"empty images {tuple(shape)}")
    if padding == "valid" and (h < 11 or w < 11):
        raise ValueError(f'padding="valid" needs H and W >= 11 (the window), got {h} x {w}; padding="same" takes any size')
    if not 0.0 <= float(ssim_lambda) <= 1.0:
        raise ValueError(f"ssim_lambda = {ssim_lambda} not in [0, 1]")
    return _lib.ImageLoss(images, h, w, ch, float(ssim_lambda), _PADDING[padding])


def l1_ssim_loss(render: torch.Tensor, target: torch.Tensor, ssim_lambda: float = 0.2, padding: str = "valid") -> torch.Tensor:
    """(1 - ssim_lambda) * mean|render - target| + ssim_lambda * (1 - ssim(render, target, padding)) (scalar tensor), the
    loss of splatfacto and gsplat's simple_trainer; render, target [..., H, W, ch] (ch 1..4).  The L1 term is the mean over
    every element, as l1_loss; SSIM as `ssim`.  Gradient flows to `render` only."""
    if render.shape != target.shape:
        raise ValueError(f"shape mismatch {tuple(render.shape)} vs {tuple(target.shape)}")
    desc = _image_loss(render.shape, ssim_lambda, padding)
    require_device(render, target)
    return _L1SSIM.apply(_f32c(render), _f32c(target.detach()), desc)


def ssim(render: torch.Tensor, target: torch.Tensor, padding: str = "valid") -> torch.Tensor:
    """Mean SSIM of render against target (scalar tensor), images [..., H, W, ch] (ch 1..4): pytorch_msssim's
    SSIM(data_range=1.0, size_average=True) for padding="valid", the original 3DGS `ssim()` for "same" (module docstring).
    Computed as 1 - l1_ssim_loss(render, target, ssim_lambda=1); gradient flows to `render` only."""
    return 1.0 - l1_ssim_loss(render, target, 1.0, padding)


class _RGBD(torch.autograd.Function):
    """_L1SSIM's pattern under an mgs_rgbd_loss descriptor: the forward leaves the complete [..., H, W, Cr] gradient for a
    cotangent of 1 (mgs_rgbd_loss_fwd_grad), any other cotangent scales it once, a second backward recomputes it
    (mgs_rgbd_loss_bwd).  Returns (loss, terms); terms carries no gradient."""

    @staticmethod
    def forward(ctx, render, target_rgb, target_depth, mask, desc):
        L = _lib.lib()
        loss = torch.empty((), dtype=torch.float32, device=render.device)
        terms = torch.empty(4, dtype=torch.float32, device=render.device)
        ctx.mark_non_differentiable(terms)
        head = [ctypes.byref(desc), ptr(render), ptr(target_rgb), ptr(target_depth), ptr(mask)]
        if not ctx.needs_input_grad[0]:
            sized_call(L.mgs_rgbd_loss_fwd, head + [ptr(loss), ptr(terms)], render.device, cached=False)
            return loss, terms
        v_render = torch.empty_like(render)
        sized_call(L.mgs_rgbd_loss_fwd_grad, head + [ptr(loss), ptr(terms), ptr(v_render)], render.device, cached=False)
        ctx.save_for_backward(render, target_rgb, target_depth, mask)
        ctx.v_render, ctx.desc = v_render, desc
        return loss, terms

    @staticmethod
    def backward(ctx, v_loss, _v_terms):
        g = _f32c(v_loss)
        v_render, ctx.v_render = ctx.v_render, None
        if v_render is not None:
            if not _is_unit(g):
                v_render.mul_(g)
            return v_render, None, None, None, None
        # a second backward through a retained graph: autograd owns the first buffer by now
        render, target_rgb, target_depth, mask = ctx.saved_tensors
        v_render = torch.empty_like(render)
        sized_call(_lib.lib().mgs_rgbd_loss_bwd, [ctypes.byref(ctx.desc), ptr(render), ptr(target_rgb), ptr(target_depth),
                                                  ptr(mask), ptr(g), ptr(v_render)], render.device, cached=False)
        return v_render, None, None, None, None


def rgbd_loss(render: torch.Tensor, target_rgb: torch.Tensor, target_depth: torch.Tensor = None, mask: torch.Tensor = None,
              ssim_lambda: float = 0.2, depth_lambda: float = 0.0, padding: str = "valid", return_terms: bool = False):
    """The masked RGB-D training loss on the frame the renderer returns, in one pass over it (include/mgs_loss_rgbd.h):

        (1 - ssim_lambda) * mean|x - y| + ssim_lambda * (1 - ssim(x, y, padding)) + depth_lambda * D,

    x = mask * render[..., :3], y = mask * target_rgb, the mean over every element (splatfacto's masked loss: not divided by
    the mask's area); D = sum w |render[..., 3] - target_depth| / sum w over all images, w = mask where target_depth is finite
    and > 0, else 0, and D = 0 where no pixel has weight.  Under mask == 0 nothing of render or of the targets enters: NaN
    or inf there leave the loss as it is and receive a gradient of exactly 0.

    render [..., H, W, 3] or [..., H, W, 4] (RGB, then expected depth: render_mode="RGB+ED"), read in place -- a contiguous
    float32 frame is not copied, and the gradient arrives complete in its layout, the depth channel included (zeros when
    depth_lambda == 0).  target_rgb [..., H, W, 3]; target_depth [..., H, W], needed (with a four-channel render) when
    depth_lambda > 0; mask [..., H, W], float32 in [0, 1], may be soft, None: all ones.  A bool or uint8 mask is taken as
    non-zero = 1 and converted on every call: keep masks resident as float32.  Gradient flows to `render` only.
    return_terms: also a device tensor {mean|x - y|, ssim, D, sum w} for logging (D and sum w are 0 when depth_lambda == 0)."""
    if render.dim() < 3 or render.shape[-1] not in (3, 4):
        raise ValueError(f"render must be [..., H, W, 3] or [..., H, W, 4], got shape {tuple(render.shape)}")
    lead = tuple(render.shape[:-1])
    if tuple(target_rgb.shape) != lead + (3,):
        raise ValueError(f"shape mismatch: target_rgb {tuple(target_rgb.shape)} vs render {tuple(render.shape)} (wants {lead + (3,)})")
    if target_depth is not None and tuple(target_depth.shape) != lead:
        raise ValueError(f"shape mismatch: target_depth {tuple(target_depth.shape)} vs render {tuple(render.shape)} (wants {lead})")
    if mask is not None and tuple(mask.shape) != lead:
        raise ValueError(f"shape mismatch: mask {tuple(mask.shape)} vs render {tuple(render.shape)} (wants {lead})")
    depth_lambda = float(depth_lambda)
    if not (math.isfinite(depth_lambda) and depth_lambda >= 0.0):
        raise ValueError(f"depth_lambda = {depth_lambda} must be finite and >= 0")
    if depth_lambda > 0.0 and render.shape[-1] != 4:
        raise ValueError("depth_lambda > 0 needs a four-channel render (render_mode=\"RGB+ED\"): there is no depth channel")
    if depth_lambda > 0.0 and target_depth is None:
        raise ValueError("depth_lambda > 0 needs target_depth")
    d = _image_loss(lead + (3,), ssim_lambda, padding)
    desc = _lib.RgbdLoss(d.images, d.height, d.width, int(render.shape[-1]), d.ssim_weight, d.padding, depth_lambda)
    require_device(render, target_rgb, target_depth, mask)
    if mask is not None:
        mask = (mask != 0).float() if mask.dtype in (torch.bool, torch.uint8) else _f32c(mask.detach())
    depth = _f32c(target_depth.detach()) if depth_lambda > 0.0 else None
    loss, terms = _RGBD.apply(_f32c(render), _f32c(target_rgb.detach()), depth, mask, desc)
    return (loss, terms) if return_terms else loss
