"""2D part masks -> per-Gaussian class ids (include/mgs_lift.h, csrc/lift.hip): the inverse direction of the label frames.

    result = lift_labels(means, quats, scales, opacities, viewmats, Ks, W, H, masks, n_classes)
    rasterization(..., class_ids=result.class_ids, n_classes=n_classes)       # or FrameRenderer(class_ids=...), transform.py

A Gaussian's vote for class k is the sum, over all views and all pixels whose mask says k, of the weight the blend gives
it at that pixel (the linear vote of FlashSplat and its relatives); the class with the most votes wins.  Per camera the
scene is projected and binned exactly as `rasterization` does, and raster_votes_kernel walks that camera's own lists: no
[C,N,...] array exists at any time, and masks may arrive in chunks (votes= continues an earlier call; the votes are
integers, so any split of the cameras over calls gives the same bits).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import ops
from ._lib import MgsError, check_tensor, require_device
from .ops import _f32c


class LiftResult(NamedTuple):
    class_ids: Tensor       # int32 [N]: the class with the most votes, -1 where no vote exceeds min_vote
    confidence: Tensor      # float32 [N]: that vote's share of the Gaussian's total, 0 where the class is -1
    votes: Tensor           # int64 [N, n_classes]: unsigned Q32 fixed point (ops.votes_to_float); feed back as votes=


@torch.no_grad()
def lift_labels(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, viewmats: Tensor, Ks: Tensor, width: int,
                height: int, masks: Tensor, n_classes: int, *, min_vote: float = 0.0, votes: Optional[Tensor] = None,
                eps2d: float = 0.3, near_plane: float = 0.01, far_plane: float = 1e10, radius_clip: float = 0.0,
                rasterize_mode: str = "classic", radius_rule: str = "classic", camera_model: str = "pinhole",
                distortion=None, pinhole_distortion=None, _debug: Optional[list] = None) -> LiftResult:
    """means [N,3], quats [N,4], scales [N,3], opacities [N] (activated), viewmats [C,4,4], Ks [C,3,3], masks uint8 [C,H,W]
    with values 0..n_classes-1 (anything else, 255 by convention, is "no class here"; a host tensor is uploaded camera by
    camera).  The projection arguments are `rasterization`'s and must be those the masks' frames were rendered with.
    min_vote: a Gaussian whose best class has no more than this many pixels of full weight stays -1.
    votes: the votes of an earlier call on other cameras of the same scene, added to in place.
    _debug: a list that receives, per camera, the projected inputs and lists the votes were cast on."""
    require_device(means, quats, scales, opacities, viewmats, Ks, votes)
    means, quats, scales, opacities = _f32c(means.detach()), _f32c(quats.detach()), _f32c(scales.detach()), _f32c(opacities.detach())
    viewmats, Ks = _f32c(viewmats), _f32c(Ks)
    N, dev = means.shape[0], means.device
    if means.dim() != 2 or means.shape[1] != 3 or quats.shape != (N, 4) or scales.shape != (N, 3) or opacities.shape != (N,):
        raise ValueError("expected means [N,3], quats [N,4], scales [N,3], opacities [N]")
    if viewmats.dim() != 3 or viewmats.shape[1:] != (4, 4) or Ks.shape != (viewmats.shape[0], 3, 3):
        raise ValueError("expected viewmats [C,4,4], Ks [C,3,3]")
    C = viewmats.shape[0]
    width, height = int(width), int(height)
    if not torch.is_tensor(masks) or masks.dtype != torch.uint8 or tuple(masks.shape) != (C, height, width):
        raise ValueError(f"masks must be a uint8 tensor {(C, height, width)}")
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"rasterize_mode {rasterize_mode!r} not in ('classic', 'antialiased')")
    n_classes = ops.check_n_classes(n_classes)
    antialiased = rasterize_mode == "antialiased"
    rule = ops.radius_rule_id(radius_rule)
    camera = ops.camera_model_id(camera_model, distortion, pinhole_distortion)
    cam_rows = ops.lens_rows(Ks, distortion, pinhole_distortion) if camera in ops.LENS_CAMERAS else Ks
    if votes is None:
        votes = torch.zeros(N, n_classes, dtype=torch.int64, device=dev)
    else:
        check_tensor("votes", votes, torch.int64, (N, n_classes))
    tile_w, tile_h = ops.tile_grid(width, height)
    for c in range(C):
        radii, means2d, depths, conics, comp = ops.projection_fwd_raw(
            means, quats, scales, viewmats[c], cam_rows[c], width, height, float(eps2d), float(near_plane), float(far_plane),
            float(radius_clip), antialiased, opacities if rule else None, rule, camera)
        opac = opacities * comp if antialiased else opacities        # the opacity the frame's raster reads
        cap = max(1, ops._upper_bound_isects(radii, tile_w, tile_h))
        tl = ops.isect_tiles_raw(means2d, radii, depths, tile_w, tile_h, cap, conics=conics,
                                 opacities=opac)                    # tight rectangles: shorter lists, the same weights
        if int(tl.status.item()) != 0:            # (one more word on a path that has just read the bound back)
            raise MgsError(f"camera {c}: tile-intersection capacity {cap} exceeded, {int(tl.n_isect.item())} slots needed; "
                           "no vote of this camera was cast")
        mask = masks[c].to(dev).contiguous()
        ops.raster_votes_raw(tl, mask, n_classes, width, height, votes, means2d=means2d, conics=conics, opacities=opac)
        if _debug is not None:
            _debug.append(dict(means2d=means2d, conics=conics, opacities=opac, lists=tl, mask=mask))
    class_ids, confidence = ops.assign_classes(votes, min_vote)
    return LiftResult(class_ids, confidence, votes)
