"""`rasterization(...)`: the whole background-render path behind the signature nerfstudio's
splatfacto calls (gsplat 1.x `rasterization`), plus `render(...)`,
the Camera/Gaussians convenience the data-generation loop would use.

Per camera the frame is these C-ABI calls on torch's current stream:
    mgs_project_color_fwd -> mgs_isect_tiles -> mgs_rasterize_fwd        (forward)
    mgs_rasterize_bwd_det -> mgs_project_color_bwd                        (backward)
With `isect_capacity` given a batch of cameras is one call instead -- mgs_render_frames (inference,
lean_meta), or mgs_render_frames_train and mgs_render_frames_backward (training) -- and nothing is
read back from the device, so a frame (or a training step) can be captured in a HIP graph.  Without
it the intersection bound is read back once per camera to size the lists, as the reference operator
does.  Features given per Gaussian go through the gsplat-style operators of ops.py instead.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import ops
from ._lib import MgsError, require_device
from .ops import TILE_SIZE, _f32c

_MODES = ("RGB", "D", "ED", "RGB+D", "RGB+ED")


class _Meta(dict):
    """The `meta` dict of `rasterization`.  The render path keeps the per-camera tile lists on
    the device at their capacity; gsplat's flat `flatten_ids` / `isect_ids` tensors are
    materialised only if somebody asks for them (one read-back of the intersection counts)."""

    def __missing__(self, key):
        if key not in ("flatten_ids", "isect_ids") or "tile_lists" not in self:
            raise KeyError(key)
        lists = self["tile_lists"]
        if lists and lists[0].tile_ids is None:
            raise KeyError(f"{key}: this frame was rendered with lean_meta=True and keeps no tile ids")
        n_tiles = self["tile_width"] * self["tile_height"]
        tile_bits = int(n_tiles).bit_length()             # floor(log2(n_tiles)) + 1
        N = self["depths"].shape[1]
        counts = [int(c) for c in self["n_isects"].tolist()]
        flat, keys = [], []
        for c, (tl, n) in enumerate(zip(lists, counts)):
            ids = tl.flatten_ids[:n]
            flat.append(ids + c * N)
            depth_bits = self["depths"][c][ids.long()].view(torch.int32).long() & 0xFFFFFFFF
            keys.append((((c << tile_bits) | tl.tile_ids[:n].long()) << 32) | depth_bits)
        self["flatten_ids"] = torch.cat(flat)
        self["isect_ids"] = torch.cat(keys)
        return self[key]


@dataclass(frozen=True)
class _RenderConfig:
    """Everything besides the eight tensors that one rasterization() call hands _RenderSH."""
    width: int
    height: int
    sh_degree: int
    eps2d: float
    near: float
    far: float
    radius_clip: float
    antialiased: bool
    with_depth: bool
    capacity: Optional[int]     # isect_capacity: fixed list capacity (nothing read back), or None
    absgrad: bool
    tight: bool                 # tightened tile rectangles
    per_axis: bool              # the per-axis (gsplat >= 1.5) radius rule
    camera: int                 # MGS_CAMERA_*
    expected_depth: bool        # "ED" modes: the raster divides the depth channel by max(alpha, 1e-10)
    latency: bool               # raster_schedule "latency"
    lean: bool                  # lean_meta
    segment: int                # backward_segment
    dataset: Optional[tuple]    # dataset_out
    raw: bool = False           # raw_params: scales are log-scales, opacities logits (MGS_PARAMS_RAW)
    labels: Optional[tuple] = None   # (class_ids int32 [N], n_classes): a label frame per camera (include/mgs_labels.h)
    hybrid: Optional[tuple] = None   # (fg_rgb [C,H,W,3], fg_depth [C,H,W], backdrop [3] | None): include/mgs_hybrid.h

    @property
    def channels(self) -> int:
        return 4 if self.with_depth else 3


class _Camera(NamedTuple):
    """What the forward keeps of one camera for the backward and the meta dict."""
    radii: Tensor               # [N], or planar [2,N] under the per-axis rule
    means2d: Tensor
    depths: Tensor
    conics: Tensor
    opac_aa: Optional[Tensor]   # the opacity the raster saw, when it is not the parameter: antialiased, or raw form
    feats: Tensor
    lists: ops.TileLists
    splats: Tensor
    checkpoints: Optional[Tensor]


def _stk(xs):
    """[C,...] of C per-camera tensors (no copy for the common single-camera call)."""
    return xs[0].unsqueeze(0) if len(xs) == 1 else torch.stack(xs)


def _hybrid_buffers(C, height, width, dev):
    """The three frames rasterization(foreground=) publishes, as the meta entries that hold them."""
    return dict(hybrid_rgb=torch.empty(C, height, width, 3, dtype=torch.float32, device=dev),
                hybrid_depth=torch.empty(C, height, width, dtype=torch.float32, device=dev),
                fg_visibility=torch.empty(C, height, width, dtype=torch.float32, device=dev))


def _hybrid_camera(cfg: "_RenderConfig", cam: "_Camera", opacities, render, alphas, c: int, out: dict) -> None:
    """mgs_raster_over_opaque on the arrays and lists camera c's raster has just read (its opacity: anti-aliased or
    activated where the frame's is), into frame c of `out`."""
    fg_rgb, fg_depth, backdrop = cfg.hybrid
    opac = cam.opac_aa if (cfg.antialiased or cfg.raw) else opacities.detach()
    ops.raster_over_opaque_raw(cam.lists, cam.means2d, cam.conics, opac, cam.feats, cam.depths, fg_rgb[c], fg_depth[c],
                               render[c], alphas[c], cfg.width, cfg.height, backdrop=backdrop,
                               out=(out["hybrid_rgb"][c], out["hybrid_depth"][c], out["fg_visibility"][c]))


class _RenderSH(torch.autograd.Function):
    """SH-coloured frames for C cameras: fused projection+colour, binning, raster."""

    @staticmethod
    def forward(ctx, means, quats, scales, opacities, sh_coeffs, viewmats, Ks, backgrounds, cfg: _RenderConfig, meta_out):
        C = viewmats.shape[0]
        dev = means.device
        width, height, ch, cap = cfg.width, cfg.height, cfg.channels, cfg.capacity
        tile_w, tile_h = ops.tile_grid(width, height)
        render = torch.empty(C, height, width, ch, dtype=torch.float32, device=dev)
        alphas = torch.empty(C, height, width, dtype=torch.float32, device=dev)
        # last_ids (and the backward's slot map) only when some input wants a gradient
        training = any(ctx.needs_input_grad[:6]) or ctx.needs_input_grad[7]
        last_ids = (torch.empty(C, height, width, dtype=torch.int32, device=dev) if training
                    else None)
        ctx.cfg, ctx.meta_out = cfg, meta_out
        lab = lab_w = None
        if cfg.labels is not None:          # the label frames: outputs that carry no gradient, published in the meta dict
            lab = torch.empty(C, height, width, dtype=torch.uint8, device=dev)
            lab_w = torch.empty(C, height, width, dtype=torch.float32, device=dev)
            meta_out["label_frames"] = dict(labels=lab, label_weights=lab_w)
        hyb = None
        if cfg.hybrid is not None:          # the exact composite with an opaque foreground: no gradient either
            hyb = meta_out["hybrid_frames"] = _hybrid_buffers(C, height, width, dev)
        ctx.set_materialize_grads(False)       # an unused output's cotangent arrives as None, not as a zero frame
        # lean: an inference frame with a fixed list capacity keeps only what its own kernels read -- the packed
        # records, the binning seed and the depths; radii / means2d / conics / feats / tiles_per_gauss are neither
        # written nor returned (36 + 4 MB of stores per 1 M Gaussians)
        lean = cfg.lean and not training and cap is not None
        if cfg.dataset is not None and not lean:
            raise ValueError("dataset_out needs inference frames through the one-call path: lean_meta=True, isect_capacity "
                             "given, no gradients")
        args = (means, quats, scales, opacities, cfg.sh_degree, sh_coeffs, viewmats, Ks, width, height, cfg.eps2d, cfg.near,
                cfg.far, cfg.radius_clip, cfg.antialiased, cfg.with_depth, cap)
        if lean:
            # the whole batch of cameras behind ONE C call (mgs_render_frames): per-camera scratch is reused, nothing
            # per Gaussian is returned
            ds = cfg.dataset
            _, _, n_isects, status = ops.render_frames_raw(
                *args, backgrounds=backgrounds, expected_last=cfg.expected_depth, latency=cfg.latency, out=(render, alphas),
                tight=cfg.tight, per_axis=cfg.per_axis, camera=cfg.camera, dataset=ds[:3] if ds is not None else None,
                float_frame=ds is None or bool(ds[3]), raw=cfg.raw,
                labels=cfg.labels + (lab, lab_w) if cfg.labels is not None else None)
            meta_out["lean"] = dict(n_isects=n_isects, isect_status=status)
            return render, alphas.unsqueeze(-1)
        if training and cap is not None:
            # the whole batch of training cameras behind ONE C call (mgs_render_frames_train): what the backward and the
            # meta dict need stays per camera in one state buffer; no read-back, so the step captures in a HIP graph
            _, _, st = ops.render_frames_train_raw(
                *args, cfg.segment, backgrounds=backgrounds, expected_last=cfg.expected_depth, latency=cfg.latency,
                tight=cfg.tight, out=(render, alphas), per_axis=cfg.per_axis, camera=cfg.camera, raw=cfg.raw)
            per_cam = []
            for c in range(C):
                v = st.views(c)
                per_cam.append(_Camera(torch.stack([v["radii"], v["radii_y"]]) if cfg.per_axis else v["radii"], v["means2d"],
                                       v["depths"], v["conics"], v["opac_aa"] if (cfg.antialiased or cfg.raw) else None, v["feats"],
                                       st.tile_lists(c, v), v["splats"], None))
                if lab is not None:         # on the camera's own records and lists, kept in the state
                    ops.raster_labels_raw(per_cam[c].lists, *cfg.labels, width, height, splats=v["splats"], out=(lab[c], lab_w[c]))
                if hyb is not None:
                    _hybrid_camera(cfg, per_cam[c], opacities, render, alphas, c, hyb)
            ctx.train_state = st
            ctx.save_for_backward(means, quats, scales, opacities, sh_coeffs, viewmats, Ks, backgrounds, alphas, None, render)
            meta_out["per_cam"] = per_cam
            return render, alphas.unsqueeze(-1)
        ctx.train_state = None
        per_cam = []
        for c in range(C):
            # the projection kernel also seeds the binning (tile rectangle + count per Gaussian)
            radii, means2d, depths, conics, opac_aa, feats, splats, seed = ops.project_color_fwd_raw(
                means, quats, scales, opacities, cfg.sh_degree, sh_coeffs, viewmats[c], Ks[c], width, height, cfg.eps2d,
                cfg.near, cfg.far, cfg.radius_clip, cfg.antialiased, cfg.with_depth, want_splats=True,
                bin_seed="tight" if cfg.tight else "classic", per_axis=cfg.per_axis, camera=cfg.camera, raw=cfg.raw)
            opac = opac_aa if (cfg.antialiased or cfg.raw) else opacities
            cam_cap = cap if cap is not None else max(1, ops._upper_bound_isects(radii, tile_w, tile_h))
            # training: these records are the ones the backward gets (_Camera.splats), so it may read their slot words
            tl = ops.isect_tiles_raw(means2d, radii, depths, tile_w, tile_h, cam_cap, c, C, want_pair_info=training,
                                     conics=conics if cfg.tight else None, opacities=opac if cfg.tight else None,
                                     seed=seed, splats=splats if training else None)
            # training: the forward leaves per-pixel checkpoints every `segment` list entries, so that the backward
            # can walk a tile's list as independent segments (include/mgs.h: mgs_rasterize_fwd)
            # (without a fixed capacity `cam_cap` is the loose bound read back above -- several times the lists: the
            #  checkpoints are then sized by the count the binning has just written, one more read-back on a path that
            #  reads back anyway)
            ckpt = None
            if training and cfg.segment:
                ckpt_cap = cam_cap if cap is not None else min(cam_cap, int(tl.n_isect.item()) + 1)
                ckpt = ops.checkpoint_buffer(ckpt_cap, tile_w, tile_h, ch, cfg.segment, dev)
            ops.rasterize_fwd_raw(means2d, conics, feats, opac,
                                  backgrounds[c] if backgrounds is not None else None, width,
                                  height, tile_w, tile_h, tl.tile_offsets, tl.flatten_ids,
                                  out=(render[c], alphas[c], last_ids[c] if training else None),
                                  splats=splats, expected_last=cfg.expected_depth, latency=cfg.latency,
                                  group_order=tl.group_order, channels=ch, checkpoints=ckpt,
                                  checkpoint_interval=cfg.segment if ckpt is not None else 0)
            if lab is not None:             # the records the raster has just read: its opacity, its lists, its launch order
                ops.raster_labels_raw(tl, *cfg.labels, width, height, splats=splats, out=(lab[c], lab_w[c]))
            per_cam.append(_Camera(radii, means2d, depths, conics, opac_aa, feats, tl, splats, ckpt))
            if hyb is not None:             # the frame just written, blended again up to the foreground's depth
                _hybrid_camera(cfg, per_cam[c], opacities, render, alphas, c, hyb)
        ctx.per_cam = per_cam
        # "RGB+ED": the kernel's epilogue divided the depth channel by max(alpha, 1e-10); the
        # backward undoes that with the saved frame (an OUTPUT: it must go through
        # save_for_backward -- parked on ctx it forms a reference cycle that crashes HIP graph capture)
        ctx.save_for_backward(means, quats, scales, opacities, sh_coeffs, viewmats, Ks,
                              backgrounds, alphas, last_ids,
                              render if ((cfg.expected_depth or cfg.segment) and training) else None)
        meta_out["per_cam"] = per_cam
        return render, alphas.unsqueeze(-1)

    @staticmethod
    def backward(ctx, v_render, v_alphas):
        (means, quats, scales, opacities, sh_coeffs, viewmats, Ks, backgrounds, alphas,
         last_ids, render_out) = ctx.saved_tensors
        cfg = ctx.cfg
        C = viewmats.shape[0]
        # set_materialize_grads(False): an output the loss does not use arrives as None instead of a zero frame
        if v_render is None:
            v_render = torch.zeros(C, cfg.height, cfg.width, cfg.channels, dtype=torch.float32, device=means.device)
        v_render = _f32c(v_render)
        v_alphas = _f32c(v_alphas).reshape(C, cfg.height, cfg.width) if v_alphas is not None else None
        if ctx.train_state is not None:
            # the batch's backward behind one C call (mgs_render_frames_backward): same kernels, same order
            v_means, v_quats, v_scales, v_sh, v_opacities, v_viewmats, v_m2d, v_abs = ops.render_frames_backward_raw(
                means, quats, scales, opacities, cfg.sh_degree, sh_coeffs, viewmats, Ks, cfg.eps2d, backgrounds,
                ctx.train_state, render_out, alphas, v_render, v_alphas, absgrad=cfg.absgrad,
                want_viewmats=ctx.needs_input_grad[5], raw=cfg.raw)
        else:
            tile_w, tile_h = ops.tile_grid(cfg.width, cfg.height)
            # "RGB+ED": the raster backward's prologue undoes the divide by max(alpha, 1e-10) itself
            # (expected_render=...); only a background gradient needs the converted cotangent
            # the first camera overwrites the outputs, later ones accumulate: no zero-fill pass
            v_means = torch.empty_like(means)
            v_quats = torch.empty_like(quats)
            v_scales = torch.empty_like(scales)
            v_sh = torch.empty_like(sh_coeffs)
            # (the opacity the raster saw is not the parameter: the blend's gradient goes through project_color_bwd_raw)
            own_opac = cfg.antialiased or cfg.raw
            v_opacities = torch.empty_like(opacities) if own_opac else None
            # camera-pose gradients only when asked for (float atomics into a zeroed [C,4,4])
            v_viewmats = torch.zeros_like(viewmats) if ctx.needs_input_grad[5] else None
            v_m2d, v_abs, blend = [], [], []
            for c, cam in enumerate(ctx.per_cam):
                opac = cam.opac_aa if own_opac else opacities
                ckpt = cam.checkpoints
                v_means2d, v_conics, v_feats, v_opac, v_means2d_abs = ops.rasterize_bwd_det_raw(
                    cam.means2d, cam.conics, cam.feats, opac, backgrounds[c] if backgrounds is not None else None, cfg.width,
                    cfg.height, tile_w, tile_h, cam.lists, alphas[c], last_ids[c], v_render[c],
                    v_alphas[c] if v_alphas is not None else None, cfg.absgrad, splats=cam.splats,
                    expected_render=render_out[c] if cfg.expected_depth else None,
                    render_out=render_out[c] if ckpt is not None else None, checkpoints=ckpt,
                    checkpoint_interval=cfg.segment if ckpt is not None else 0)
                v_m2d.append(v_means2d)
                v_abs.append(v_means2d_abs)
                # (all four blend-stage gradients, for tests that gate the raster backward on its own)
                blend.append((v_means2d, v_conics, v_feats, v_opac))
                ops.project_color_bwd_raw(
                    means, quats, scales, opacities, cfg.sh_degree, sh_coeffs, viewmats[c], Ks[c], cfg.width, cfg.height,
                    cfg.eps2d, cam.radii, cam.conics, cfg.antialiased, cam.feats, v_feats, v_means2d, v_conics,
                    v_opac if own_opac else None, v_means, v_quats, v_scales, v_sh, v_opacities,
                    v_viewmats[c] if v_viewmats is not None else None, accumulate=c > 0, camera=cfg.camera, raw=cfg.raw)
                if not own_opac:
                    v_opacities = v_opac if v_opacities is None else v_opacities + v_opac
            ctx.meta_out["blend_grads"] = blend
        # screen-space gradients for densification strategies: published in the meta dict, and gsplat users call
        # meta["means2d"].retain_grad() and read .grad / .absgrad after backward -- meta["means2d"] is handed out as a
        # leaf that receives them here.  v_m2d / v_abs: [C,N,2] (one call) or lists of C [N,2] (per camera)
        meta = ctx.meta_out
        meta["means2d_grad"] = list(v_m2d)
        if cfg.absgrad:
            meta["means2d_absgrad"] = list(v_abs)
        m2d = meta.get("means2d")
        if m2d is not None and m2d.requires_grad:
            m2d.grad = v_m2d if torch.is_tensor(v_m2d) else _stk(v_m2d)
            if cfg.absgrad:
                m2d.absgrad = v_abs if torch.is_tensor(v_abs) else _stk(v_abs)
        v_bg = None
        if backgrounds is not None and ctx.needs_input_grad[7]:
            if cfg.expected_depth:
                v_render = torch.cat([v_render[..., :-1],
                                      (v_render[..., -1] / alphas.clamp(min=1e-10)).unsqueeze(-1)], dim=-1)
            v_bg = (v_render * (1.0 - alphas).unsqueeze(-1)).sum(dim=(1, 2))
        return v_means, v_quats, v_scales, v_opacities, v_sh, v_viewmats, None, v_bg, None, None


def rasterization(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor,
                  colors: Tensor, viewmats: Tensor, Ks: Tensor, width: int, height: int,
                  near_plane: float = 0.01, far_plane: float = 1e10, radius_clip: float = 0.0,
                  eps2d: float = 0.3, sh_degree: Optional[int] = None, packed: bool = False,
                  tile_size: int = TILE_SIZE, backgrounds: Optional[Tensor] = None,
                  render_mode: str = "RGB", sparse_grad: bool = False, absgrad: bool = False,
                  rasterize_mode: str = "classic", channel_chunk: int = 32,
                  isect_capacity: Optional[int] = None,
                  tile_bounds: str = "tight",
                  raster_schedule: str = "latency",
                  lean_meta: bool = False,
                  backward_segment: int = 256,
                  radius_rule: str = "classic",
                  dataset_out=None,
                  camera_model: str = "pinhole",
                  distortion=None,
                  pinhole_distortion=None,
                  raw_params: bool = False,
                  class_ids: Optional[Tensor] = None,
                  n_classes: Optional[int] = None,
                  foreground: Optional[Tuple[Tensor, Tensor]] = None,
                  backdrop=None) -> Tuple[Tensor, Tensor, Dict]:
    """Render N Gaussians from C cameras.

    foreground = (fg_rgb [C,H,W,3], fg_depth [C,H,W]), an opaque layer as rasterize_mesh returns it (rendered to match:
    under distortion= / pinhole_distortion= give rasterize_mesh the same camera_model and coefficients, and the two layers
    register pixel for pixel; z-depth, 0 where no
    face is), with render_mode="RGB+ED": every frame also gets its exact composite with that layer (include/mgs_hybrid.h,
    DESIGN.md 4.17) -- meta["hybrid_rgb"] [C,H,W,3] and meta["hybrid_depth"] [C,H,W], the pixel's own front-to-back blend
    stopped at the foreground's depth with the foreground entering at the transmittance reached there, and
    meta["fg_visibility"] [C,H,W], that transmittance (0 where there is no foreground; there the frame itself is copied,
    + (1 - alpha) backdrop, backdrop = three floats or None).  Where the splats at a pixel straddle the foreground --
    a table edge, foliage, a semi-transparent layer in front of the arm -- this is what composite_over's single depth
    comparison cannot give.  Colours, alphas and every other meta entry are what they are without the keyword.  On the
    per-Gaussian feature path ([N,3] / [C,N,3] colours) and on the SH path with per-camera intermediates; refused with
    lean_meta=True or dataset_out (the one-C-call frames keep nothing per Gaussian) and not part of FrameRenderer's
    captured graphs.  Under rasterize_mode="antialiased" or raw_params it blends with the opacity the raster saw.  No
    gradient.

    class_ids (any integer tensor [N] on the device) with n_classes = K <= 32: every frame also gets a part-label frame,
    meta["labels"] [C,H,W] uint8 -- the class whose Gaussians hold the largest share of the pixel's blend weights, ties to
    the lowest class, 255 where no counted Gaussian has a class in 0..K-1 -- and meta["label_weights"] [C,H,W] float32,
    that share (threshold it against alpha to decide how much coverage counts as "this part").  A class outside 0..K-1
    (-1, say) occludes and is never reported.  The weights are the frame's own blend weights bit for bit;
    colours, alphas and every other meta entry are what they are without class_ids.  On every path: per-Gaussian features,
    SH with per-camera intermediates, and lean_meta, where the label launch sits inside the one C call (graph-capturable).
    n_classes=None reads class_ids.max() back once -- not under graph capture.  Labels carry no gradient.

    raw_params (SH path): `scales` hold log-scales and `opacities` logits -- what a nerfstudio .ply stores and
    splatfacto's optimiser steps on -- and the returned gradients are with respect to those tensors.  The projection
    kernels apply exp / sigmoid in registers (include/mgs.h MGS_PARAMS_RAW) and their backward applies the two chain-rule
    factors: no activation launches, no activated copies, no autograd nodes between the optimiser's leaves and the
    renderer.  Everything else is as in the activated form; meta["opacities"] stays post-activation [C,N].

    dataset_out = (rgba uint8 [C,H,W,4], distance [C,H,W,1] float16 / 32 / 64 or None, K [3,3], keep_float_frame):
    inference frames ("RGB+ED", lean_meta=True, isect_capacity given) leave the raster as the dataset frames the
    reference's readers open (dataset.frame_to_dataset's bytes) in the caller's buffers; with keep_float_frame False the
    float frame is not written at all and the returned colours / alphas are unspecified.

    radius_rule: "classic" -- gsplat 1.4's single radius ceil(3 sqrt(lambda_1)) per Gaussian (the
    semantics this build's parity claim is made for) -- or "opacity_aware" -- gsplat >= 1.5's per-axis extents
    min(3.33, sqrt(2 ln(255 opacity))) sqrt(Sigma_ii): meta["radii"] is then [C,N,2], Gaussians of
    opacity < 1/255 are culled, n_isect shrinks and pixels change in the corners of the classic square and beyond
    3 sigma of opaque Gaussians.  A compile-time policy of the projection kernels (both instantiations ship).

    camera_model: "pinhole", "ortho" (fx x + cx, fy y + cy) or "fisheye" (ideal equidistant lens, r = f theta, no
    distortion coefficients), gsplat's names; include/mgs.h MGS_CAMERA_* gives the maps.  Every path honours it (a
    compile-time policy of the projection kernels, like the radius rule).  Depths stay camera z and the SH view
    direction mean - campos under every model.  dataset_out is pinhole-only (its ray distance is pinhole's).

    distortion (camera_model="fisheye" only, else ValueError): the lens's OpenCV fisheye coefficients k1..k4 as host data,
    a sequence or ndarray [4] (one lens) or [C,4] (one per camera) -- cv2.fisheye / nerfstudio OPENCV_FISHEYE:
    theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8).  Projection, Jacobian and every gradient are
    the lens's (include/mgs.h MGS_CAMERA_FISHEYE_KB, a fourth instantiation of the projection kernels); a Gaussian past
    theta_max, where the polynomial stops growing (camera.lens_theta_max, computed here on the host), is culled like one
    behind the near plane.  None or all zero: the ideal lens, bit for bit the call without the keyword.  meta is unchanged.

    pinhole_distortion (camera_model="pinhole" only, else ValueError; not together with distortion= or dataset_out): the
    lens of a calibrated pinhole camera, OpenCV's distCoeffs k1 k2 p1 p2 k3 as host data, a sequence or ndarray [5] (one
    lens; [4]: k3 = 0) or [C,5] (one per camera) -- cv2.calibrateCamera / nerfstudio OPENCV: with x' = x/z, y' = y/z,
    u = x'^2 + y'^2, Rad = 1 + k1 u + k2 u^2 + k3 u^3, the pixel is (fx xd + cx, fy yd + cy) at
    xd = x' Rad + 2 p1 x' y' + p2 (u + 2 x'^2), yd = y' Rad + p1 (u + 2 y'^2) + 2 p2 x' y'.  Projection, Jacobian and every
    gradient are the lens's (include/mgs_lens_pinhole.h MGS_CAMERA_PINHOLE_BC, a fifth instantiation of the projection
    kernels).  The Jacobian is not clamped; instead a Gaussian is culled like one behind the near plane when its centre
    lies past the radial fold (u >= u_max, camera.pinhole_lens_u_max, computed here on the host), where the lens map folds
    (det of its 2 x 2 Jacobian <= 0), or when the distorted centre lies outside the frame grown by 0.3 of the half field
    -- the box the plain pinhole clamps its Jacobian to.  That last cull is the one difference from the plain pinhole
    besides the lens: a Gaussian centred outside the box is dropped rather than kept with a clamped J.  None or all zero:
    no lens, bit for bit the call without the keyword.  meta is unchanged.

    backward_segment (SH path, when gradients are wanted): list entries per unit of work of the backward raster
    (a power of two >= 64; 0 = one unit per tile, the whole-list walk).  The training forward stores per-pixel
    checkpoints at that interval ((1 + channels) * 1 KB per tile and segment) and the backward walks the segments
    independently: no tile is one wave's serial job any more.  Gradients equal the whole-list walk's up to rounding.

    lean_meta (SH path, isect_capacity given, no gradients): all C cameras go through ONE C call
    (mgs_render_frames) whose frames keep only what their own kernels read; meta then holds n_isects and
    isect_status [C] and nothing per Gaussian or per tile, and the projection kernel skips 40 MB of stores per
    1 M Gaussians.  FrameRenderer's default.

    raster_schedule (SH path): "latency" runs the tile raster with one wave per 8x8 block (the launch
    has the GPU to itself: a single frame, a training step; -19 % kernel time), "throughput" with
    one wave per tile (7 % fewer vector instructions: several independent frames in flight, where
    other frames' kernels fill the gaps anyway -- FrameRenderer picks it when frames_in_flight > 1).
    The pixels are identical bit for bit.

    tile_bounds (SH path): "tight" bins each Gaussian only into the tiles it can reach with
    alpha >= 1/255 (mgs_isect_tiles with conics + opacities): same image and gradients bit for
    bit, shorter lists; meta["tiles_per_gauss"] / ["n_isects"] then count those lists.
    "classic" reproduces gsplat's mean +- radius rectangles in the meta outputs as well.

    means [N,3], quats [N,4] (wxyz), scales [N,3], opacities [N] (post-activation);
    colors [N,K,3] SH coefficients when sh_degree is given, else [N,D] / [C,N,D] features;
    viewmats [C,4,4] OpenCV world-to-camera; Ks [C,3,3].
    Returns render_colors [C,H,W,D'], render_alphas [C,H,W,1], meta.
    """
    if render_mode not in _MODES:
        raise ValueError(f"render_mode {render_mode!r} not in {_MODES}")
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"rasterize_mode {rasterize_mode!r}")
    if packed or sparse_grad:
        raise NotImplementedError("packed / sparse_grad are not supported")
    if tile_size != TILE_SIZE:
        raise NotImplementedError(f"tile_size must be {TILE_SIZE}")
    if raw_params and sh_degree is None:
        raise NotImplementedError("raw_params needs sh_degree: per-Gaussian features run gsplat's post-activation operators")
    if tile_bounds not in ("tight", "classic"):
        raise ValueError(f"tile_bounds {tile_bounds!r} not in ('tight', 'classic')")
    rule = ops.radius_rule_id(radius_rule)
    camera = ops.camera_model_id(camera_model, distortion, pinhole_distortion)
    if dataset_out is not None and pinhole_distortion is not None:
        raise ValueError("dataset_out converts depth to ray distance through an undistorted pinhole K^-1: there is no "
                         "dataset output with pinhole_distortion=")
    if dataset_out is not None and camera != 0:
        raise ValueError(f"dataset_out converts depth to ray distance through a pinhole K^-1: camera_model "
                         f"{camera_model!r} has no dataset output")
    if backward_segment and (backward_segment < 64 or backward_segment & (backward_segment - 1)):
        raise ValueError(f"backward_segment {backward_segment} is not 0 or a power of two >= 64")
    if raster_schedule not in ("latency", "throughput"):
        raise ValueError(f"raster_schedule {raster_schedule!r} not in ('latency', 'throughput')")
    require_device(means, quats, scales, opacities, colors, viewmats, Ks, backgrounds)
    N, C = means.shape[0], viewmats.shape[0]
    labels = None
    if class_ids is not None:
        cls = ops.class_ids_i32(class_ids, N)
        if n_classes is None:
            if torch.cuda.is_current_stream_capturing():
                raise ValueError("n_classes=None reads class_ids.max() back to the host, which a graph capture cannot do: "
                                 "give n_classes")
            n_classes = int(cls.max().item()) + 1 if N > 0 else 1
        labels = (cls, ops.check_n_classes(n_classes))
    elif n_classes is not None:
        raise ValueError("n_classes given without class_ids")
    hybrid = None
    if foreground is not None:
        if render_mode != "RGB+ED":
            raise ValueError(f"foreground= composites colour and expected depth: it needs render_mode='RGB+ED', not {render_mode!r}")
        if lean_meta or dataset_out is not None:
            raise ValueError("foreground= blends each camera's own arrays and lists again, which lean_meta=True / dataset_out "
                             "frames do not keep: render without them (FrameRenderer's graphs do not carry this operator)")
        fg_rgb, fg_depth = foreground
        require_device(fg_rgb, fg_depth)
        if tuple(fg_rgb.shape) != (C, int(height), int(width), 3) or tuple(fg_depth.shape) != (C, int(height), int(width)):
            raise ValueError(f"foreground must be (fg_rgb {(C, int(height), int(width), 3)}, fg_depth {(C, int(height), int(width))}), "
                             f"got {tuple(fg_rgb.shape)} and {tuple(fg_depth.shape)}")
        hybrid = (_f32c(fg_rgb.detach()), _f32c(fg_depth.detach()), ops.backdrop_f32(backdrop, means.device))
    elif backdrop is not None:
        raise ValueError("backdrop given without foreground")
    if means.shape != (N, 3) or quats.shape != (N, 4) or scales.shape != (N, 3) \
            or opacities.shape != (N,):
        raise ValueError("expected means [N,3], quats [N,4], scales [N,3], opacities [N]")
    if viewmats.shape != (C, 4, 4) or Ks.shape != (C, 3, 3):
        raise ValueError("expected viewmats [C,4,4], Ks [C,3,3]")
    means, quats, scales, opacities = _f32c(means), _f32c(quats), _f32c(scales), _f32c(opacities)
    colors, viewmats, Ks, backgrounds = _f32c(colors), _f32c(viewmats), _f32c(Ks), _f32c(backgrounds)
    lens_rows = ops.lens_rows(Ks, distortion, pinhole_distortion) if camera in ops.LENS_CAMERAS else None
    width, height = int(width), int(height)
    antialiased = rasterize_mode == "antialiased"
    want_rgb = render_mode.startswith("RGB")
    want_depth = render_mode != "RGB"
    tile_w, tile_h = ops.tile_grid(width, height)
    meta: Dict = _Meta({"width": width, "height": height, "tile_size": TILE_SIZE,
                        "tile_width": tile_w, "tile_height": tile_h, "n_cameras": C,
                        "camera_ids": None, "gaussian_ids": None})

    # "D" / "ED" of an SH-coloured scene with a fixed list capacity (FrameRenderer, HIP graphs): the fused,
    # read-back-free path renders RGB + depth and the depth channel is sliced off below
    depth_only_via_sh = (sh_degree is not None and not want_rgb and isect_capacity is not None
                         and colors.dim() == 3 and colors.shape[-1] == 3)
    if depth_only_via_sh and backgrounds is not None:
        if backgrounds.shape != (C, 1):
            raise ValueError("backgrounds must be [C, channels]")
        backgrounds = torch.cat([backgrounds.new_zeros(C, 3), backgrounds], dim=-1)
    if sh_degree is not None and (want_rgb or depth_only_via_sh):
        if colors.dim() != 3 or colors.shape[0] != N or colors.shape[2] != 3:
            raise ValueError("with sh_degree set, colors must be [N,K,3]")
        if not 0 <= sh_degree <= 3 or colors.shape[1] < (sh_degree + 1) ** 2:
            raise ValueError("sh_degree outside 0..3 or too few coefficients")
        if backgrounds is not None and backgrounds.shape != (C, 4 if want_depth else 3):
            raise ValueError("backgrounds must be [C, channels]")
        cfg = _RenderConfig(
            width, height, int(sh_degree), float(eps2d), float(near_plane), float(far_plane), float(radius_clip),
            antialiased, want_depth, isect_capacity, bool(absgrad), tight=tile_bounds == "tight", per_axis=bool(rule),
            camera=camera, expected_depth=render_mode in ("RGB+ED", "ED"), latency=raster_schedule == "latency",
            lean=bool(lean_meta), segment=int(backward_segment), dataset=dataset_out, raw=bool(raw_params),
            labels=labels, hybrid=hybrid)
        # the autograd function publishes per-camera intermediates (and, after backward, "means2d_grad" /
        # "means2d_absgrad" lists) into the meta dict
        # (under the lens the kernels read the cameras' 16-float rows where they read K otherwise)
        render, alphas = _RenderSH.apply(means, quats, scales, opacities, colors, viewmats,
                                         Ks if lens_rows is None else lens_rows, backgrounds, cfg, meta)
        if depth_only_via_sh:
            render = render[..., 3:4]
        if "label_frames" in meta:
            meta.update(meta.pop("label_frames"))
        if "hybrid_frames" in meta:
            meta.update(meta.pop("hybrid_frames"))
        if "lean" in meta:              # inference frames through mgs_render_frames: counts and status only
            meta.update(meta.pop("lean"))
            return render, alphas, meta
        per_cam = meta.pop("per_cam")

        def _cat(xs):
            return xs[0] if len(xs) == 1 else torch.cat(xs)
        meta.update(
            radii=_stk([ops.radii_meta(p.radii) for p in per_cam]),
            means2d=_stk([p.means2d for p in per_cam]),
            conics=_stk([p.conics for p in per_cam]),
            tiles_per_gauss=_stk([p.lists.tiles_per_gauss for p in per_cam]),
            depths=_stk([p.depths for p in per_cam]),
            opacities=(_stk([p.opac_aa for p in per_cam]) if (antialiased or raw_params)
                       else opacities.unsqueeze(0).expand(C, N)),
            n_isects=_cat([p.lists.n_isect for p in per_cam]),
            isect_status=_cat([p.lists.status for p in per_cam]),
            isect_offsets=_stk([p.lists.tile_offsets[:-1].view(tile_h, tile_w) for p in per_cam]),
            tile_lists=[p.lists for p in per_cam])
        if torch.is_grad_enabled() and render.requires_grad and "means2d" in meta:
            meta["means2d"] = meta["means2d"].detach().requires_grad_(True)   # see _RenderSH.backward
    else:
        # feature path: colours are given per Gaussian (or evaluated from SH for "D"/"ED")
        if raw_params:
            raise NotImplementedError("raw_params needs the fused SH colour path (an RGB mode, or isect_capacity for 'D' / 'ED'): "
                                      "this path runs gsplat's post-activation operators")
        if isect_capacity is not None:
            # this path sizes its lists by reading the intersection count back (as the reference
            # operator does), so it can neither honour a fixed capacity nor be captured in a graph
            raise NotImplementedError(
                "isect_capacity (read-back-free, graph-capturable frames) needs the SH colour path "
                "(sh_degree given with [N,K,3] coefficients); drop isect_capacity for per-Gaussian features")
        radii, means2d, depths, conics, comps = ops.fully_fused_projection(
            means, None, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane,
            radius_clip, calc_compensations=antialiased, opacities=opacities if rule else None,
            radius_rule=radius_rule, camera_model=camera_model, distortion=distortion,
            pinhole_distortion=pinhole_distortion)
        opac = opacities.unsqueeze(0).expand(C, N)
        if antialiased:
            opac = opac * comps
        feats = None
        if want_rgb:
            feats = colors.unsqueeze(0).expand(C, N, -1) if colors.dim() == 2 else colors
            if feats.shape[:2] != (C, N):
                raise ValueError("colors must be [N,D] or [C,N,D] when sh_degree is None")
        if want_depth:
            d = depths.unsqueeze(-1)
            feats = d if feats is None else torch.cat([feats, d], dim=-1)
        tpg, isect_ids, flatten_ids = ops.isect_tiles(means2d, radii, depths, TILE_SIZE, tile_w,
                                                      tile_h)
        offsets = ops.isect_offset_encode(isect_ids, C, tile_w, tile_h)
        render, alphas = ops.rasterize_to_pixels(means2d, conics, feats.contiguous(),
                                                 opac.contiguous(), width, height, TILE_SIZE,
                                                 offsets, flatten_ids, backgrounds=backgrounds,
                                                 absgrad=absgrad)
        meta.update(radii=radii, means2d=means2d, depths=depths, conics=conics, opacities=opac,
                    tiles_per_gauss=tpg, isect_ids=isect_ids, flatten_ids=flatten_ids,
                    isect_offsets=offsets)
        if labels is not None:
            meta["labels"], meta["label_weights"] = ops.rasterize_labels(
                means2d, conics, opac.contiguous(), labels[0], labels[1], width, height, TILE_SIZE, offsets, flatten_ids,
                return_weights=True)
        if render_mode in ("ED", "RGB+ED"):      # operator path (explicit features): divide here
            render = torch.cat([render[..., :-1],
                                render[..., -1:] / alphas.clamp(min=1e-10)], dim=-1)
        if hybrid is not None:                   # on the divided frame: where there is no foreground it is copied
            if feats.shape[-1] != 4:
                raise ValueError("foreground= needs three colour channels: colors [N,3] or [C,N,3]")
            meta["hybrid_rgb"], meta["hybrid_depth"], meta["fg_visibility"] = ops.rasterize_over_opaque(
                means2d, conics, feats, depths, opac, hybrid[0], hybrid[1], render, alphas, width, height, TILE_SIZE, offsets,
                flatten_ids, backdrop=hybrid[2], return_visibility=True)
    return render, alphas, meta


def check_isect_status(meta: Dict) -> None:
    """Raise if any camera's intersection list overflowed its capacity (reads one word back)."""
    if "isect_status" in meta and bool((meta["isect_status"] != 0).any().item()):
        need = int(meta["n_isects"].max().item())
        raise MgsError(f"tile-intersection capacity exceeded: a camera needs {need} slots; "
                            "re-render with a larger isect_capacity")


def render(gaussians, cameras: Sequence, sh_degree: Optional[int] = None,
           render_mode: str = "RGB+ED", background: Optional[Sequence[float]] = None,
           device: str = "cuda", tensors: Optional[Dict] = None, **kw):
    """Render a `Gaussians` scene from `Camera`s (the Python-side API that stays, per the
    north star).  Applies splatfacto's post-processing: rgb = clamp(rgb + (1-alpha)*bg, 0, 1),
    depth = where(alpha > 0, depth, max depth).  Returns dict(rgb, depth, alpha, meta), and with class_ids= / n_classes=
    (rasterization's keywords) also labels [C,H,W] uint8 and label_weights [C,H,W]."""
    cams = list(cameras)
    w, h = cams[0].width, cams[0].height
    if any(c.width != w or c.height != h for c in cams):
        raise ValueError("all cameras of one call must share a resolution")
    if any(c.model != cams[0].model for c in cams):
        raise ValueError("all cameras of one call must share a camera model")
    kw.setdefault("camera_model", cams[0].model)
    if cams[0].model == "fisheye" and any(c.distortion is not None for c in cams):
        kw.setdefault("distortion", np.array([c.distortion or (0.0,) * 4 for c in cams], dtype=np.float64))
    if cams[0].model == "pinhole" and any(c.pinhole_distortion is not None for c in cams):
        kw.setdefault("pinhole_distortion", np.array([c.pinhole_distortion or (0.0,) * 5 for c in cams], dtype=np.float64))
    t = tensors if tensors is not None else gaussians.to_torch(device, sh_degree)
    viewmats = torch.from_numpy(np.stack([c.viewmat() for c in cams]).astype(np.float32)).to(device)
    Ks = torch.from_numpy(np.stack([c.K for c in cams]).astype(np.float32)).to(device)
    colors, alphas, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"],
                                         t["colors"], viewmats, Ks, w, h,
                                         near_plane=cams[0].near, far_plane=cams[0].far,
                                         sh_degree=t["sh_degree"], render_mode=render_mode, **kw)
    out = {"alpha": alphas, "meta": meta}
    if "labels" in meta:             # class_ids= / n_classes= (forwarded through **kw): the part-label frames
        out["labels"], out["label_weights"] = meta["labels"], meta["label_weights"]
    if render_mode.startswith("RGB"):
        rgb = colors[..., :3]
        if background is not None:
            bg = torch.tensor(background, dtype=torch.float32, device=rgb.device)
            rgb = rgb + (1.0 - alphas) * bg
        out["rgb"] = rgb.clamp(0.0, 1.0)
    if render_mode != "RGB":
        depth = colors[..., -1:]
        out["depth"] = torch.where(alphas > 0, depth, depth.detach().max())
    return out
