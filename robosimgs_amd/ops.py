"""Stage operators of the render path, gsplat-1.x-compatible signatures (SURVEY.md 8(b),
Appendix A.1), each a thin torch wrapper over one C-ABI entry point of libmgs.so.

    fully_fused_projection   -> mgs_projection_fwd / mgs_projection_bwd
    spherical_harmonics      -> mgs_sh_fwd / mgs_sh_bwd
    isect_tiles              -> mgs_isect_tiles
    isect_offset_encode      -> mgs_isect_offset_encode
    rasterize_to_pixels      -> mgs_rasterize_fwd / mgs_rasterize_bwd
    rasterize_labels         -> mgs_raster_labels (include/mgs_labels.h; no gsplat counterpart, no backward)
    rasterize_votes          -> mgs_raster_votes (include/mgs_lift.h: 2D masks -> per-Gaussian class votes)
    assign_classes           -> mgs_lift_assign
    rasterize_over_opaque    -> mgs_raster_over_opaque (include/mgs_hybrid.h: the frame's blend stopped at an opaque foreground)

Inputs are post-activation fp32 CUDA(HIP) tensors (the render-path calls also take the raw form, log-scales and
opacity logits, with raw=True: include/mgs.h MGS_PARAMS_RAW); ids are int32, keys int64.  All kernels
are enqueued on torch's current stream.  Nothing here computes on the CPU.

The three operators that walk a camera's tile lists (labels, votes, over_opaque) share their host side: _walk_source and
_walk_lists check what the kernel reads through raw pointers (_lib.check_tensor), _gsplat_lists and _flat_arrays turn
gsplat's flat [C,...] arguments into per-camera raw calls.  A further walk-based operator is a wrapper around those.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._lib import aligned_workspace, check, check_tensor, ptr, require_device, sized_call, stream_handle

TILE_SIZE = 16


def tile_grid(width: int, height: int) -> Tuple[int, int]:
    """(tile_w, tile_h): the 16x16 tiles that cover a width x height frame."""
    return -(-width // TILE_SIZE), -(-height // TILE_SIZE)


def _f32c(t: Optional[Tensor]) -> Optional[Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


# ======================================================================================
# single-camera raw calls (no autograd); used by the operators below and by rendering.py
# ======================================================================================
RADIUS_RULES = {"classic": 0, "opacity_aware": 1}     # include/mgs.h MGS_RADIUS_CLASSIC / MGS_RADIUS_OPACITY_AWARE


def radius_rule_id(radius_rule) -> int:
    if radius_rule not in RADIUS_RULES:
        raise ValueError(f"radius_rule {radius_rule!r} not in {tuple(RADIUS_RULES)}")
    return RADIUS_RULES[radius_rule]


CAMERA_MODELS = {"pinhole": 0, "ortho": 1, "fisheye": 2}    # include/mgs.h MGS_CAMERA_PINHOLE / _ORTHO / _FISHEYE

# include/mgs.h flag bits, named as there without the MGS_ prefix (tests/test_abi.py checks them against the header)
RASTER_EXPECTED_LAST, RASTER_LATENCY = 1, 2              # mgs_rasterize_fwd flags (also in the mgs_render_frames* flags)
FRAMES_CLASSIC_BOUNDS, FRAMES_RADIUS_OPACITY_AWARE = 4, 8  # mgs_render_frames* flags
FRAMES_CAMERA_ORTHO, FRAMES_CAMERA_FISHEYE = 16, 32
BIN_TIGHT, BIN_RADIUS_OPACITY_AWARE = 1, 2               # mgs_project_color_fwd bin_flags
BIN_CAMERA_ORTHO, BIN_CAMERA_FISHEYE = 4, 8
RASTER_BWD_RECORDS_ONLY, RASTER_BWD_SPLAT_SLOTS = 1, 2   # mgs_rasterize_bwd_det call_flags
PARAMS_RAW = 64          # the parameter form: bin_flags, the mgs_render_frames* flags, mgs_project_color_bwd's camera word
PARAMS_OPAC_PLAIN = 128  # bin_flags, with PARAMS_RAW: opac_out keeps the plain activated opacity (not anti-aliased)
CAMERA_BIN_FLAGS = {0: 0, 1: BIN_CAMERA_ORTHO, 2: BIN_CAMERA_FISHEYE}           # MGS_CAMERA_* -> bin_flags bits
CAMERA_FRAME_FLAGS = {0: 0, 1: FRAMES_CAMERA_ORTHO, 2: FRAMES_CAMERA_FISHEYE}   # MGS_CAMERA_* -> mgs_render_frames* bits
# The lens (include/mgs_lens.h): camera_model="fisheye" with distortion coefficients is a model of its own inside the library
CAMERA_FISHEYE_KB = 3                                           # MGS_CAMERA_FISHEYE_KB
BIN_CAMERA_FISHEYE_KB = FRAMES_CAMERA_FISHEYE_KB = 256          # its bin_flags / mgs_render_frames* bit
LENS_ROW_FLOATS = 16       # floats per camera behind K / Ks under that model: K | k1..k4 | u_max | 0 0
# The pinhole lens (include/mgs_lens_pinhole.h): camera_model="pinhole" with OpenCV's k1 k2 p1 p2 k3, the fifth model
CAMERA_PINHOLE_BC = 4                                           # MGS_CAMERA_PINHOLE_BC
BIN_CAMERA_PINHOLE_BC = FRAMES_CAMERA_PINHOLE_BC = 512          # its bin_flags / mgs_render_frames* bit
LENS_CAMERAS = (CAMERA_FISHEYE_KB, CAMERA_PINHOLE_BC)           # the models whose K / Ks are 16-float rows (lens_rows)


# (In the two lookups below the tables of the three named models come last, so an entry of theirs wins over the lens's:
#  tests/test_gpu_camera_models.py puts a key 3 with two camera bits into them to reach the C ABI's both-bits error.)
def camera_bin_flags(camera) -> int:
    """MGS_CAMERA_* -> the bin_flags bits that select it."""
    return {CAMERA_FISHEYE_KB: BIN_CAMERA_FISHEYE_KB, CAMERA_PINHOLE_BC: BIN_CAMERA_PINHOLE_BC, **CAMERA_BIN_FLAGS}[int(camera)]


def camera_frame_flags(camera) -> int:
    """MGS_CAMERA_* -> the mgs_render_frames* bits that select it."""
    return {CAMERA_FISHEYE_KB: FRAMES_CAMERA_FISHEYE_KB, CAMERA_PINHOLE_BC: FRAMES_CAMERA_PINHOLE_BC,
            **CAMERA_FRAME_FLAGS}[int(camera)]


def frames_flags(expected_last, latency, tight, per_axis, camera, raw=False) -> int:
    """The flags word of mgs_render_frames / _train / _backward."""
    return ((RASTER_EXPECTED_LAST if expected_last else 0) | (RASTER_LATENCY if latency else 0)
            | (0 if tight else FRAMES_CLASSIC_BOUNDS) | (FRAMES_RADIUS_OPACITY_AWARE if per_axis else 0)
            | camera_frame_flags(camera) | (PARAMS_RAW if raw else 0))


class LensRows:
    """A lens that already sits on the device as camera rows: `rows` is a contiguous float32 [C,16] tensor in the layout
    lens_rows() builds (K | k1..k4 | u_max | 0 0, or K | k1 k2 p1 p2 k3 | u_max | 0 under the pinhole lens).  Given as
    distortion= (pinhole_distortion= for the pinhole lens) by a caller that keeps the rows in a buffer of its
    own and overwrites K in place (FrameRenderer's camera slots); the kernels then read K from the rows, not from Ks."""
    __slots__ = ("rows",)

    def __init__(self, rows: Tensor):
        self.rows = rows


def lens_coefficients(distortion, n_cams=None):
    """distortion= as the calls take it -- None, or host data (sequence / ndarray) [4] or [C,4] of OpenCV fisheye k1..k4 --
    -> None when there is no lens (None or all zero: the ideal-fisheye instantiation), else a float64 ndarray [C,4] or
    [1,4] (one lens for every camera).  A LensRows is returned as it is."""
    if distortion is None or isinstance(distortion, LensRows):
        return distortion
    if torch.is_tensor(distortion):
        if distortion.is_cuda:
            raise ValueError("distortion is host data (a sequence or ndarray [4] or [C,4]), not a device tensor")
        distortion = distortion.numpy()
    k = np.asarray(distortion, dtype=np.float64)
    if k.ndim == 1:
        k = k[None]
    if k.ndim != 2 or k.shape[1] != 4 or (n_cams is not None and k.shape[0] not in (1, int(n_cams))):
        raise ValueError(f"distortion must be [4] or [C,4] (k1..k4 per camera), got {tuple(np.shape(distortion))}")
    if not np.isfinite(k).all():
        raise ValueError("distortion coefficients must be finite")
    return k if k.any() else None


def pinhole_lens_coefficients(pinhole_distortion, n_cams=None):
    """pinhole_distortion= as the calls take it -- None, or host data (sequence / ndarray) [5] or [C,5] of OpenCV's
    distCoeffs k1 k2 p1 p2 k3 ([4] / [C,4]: k3 = 0) -- -> None when there is no lens (None or all zero: the plain pinhole
    instantiation), else a float64 ndarray [C,5] or [1,5] (one lens for every camera).  A LensRows is returned as it is."""
    if pinhole_distortion is None or isinstance(pinhole_distortion, LensRows):
        return pinhole_distortion
    if torch.is_tensor(pinhole_distortion):
        if pinhole_distortion.is_cuda:
            raise ValueError("pinhole_distortion is host data (a sequence or ndarray [5] or [C,5]), not a device tensor")
        pinhole_distortion = pinhole_distortion.numpy()
    k = np.asarray(pinhole_distortion, dtype=np.float64)
    if k.ndim == 1:
        k = k[None]
    if k.ndim != 2 or k.shape[1] not in (4, 5) or (n_cams is not None and k.shape[0] not in (1, int(n_cams))):
        raise ValueError(f"pinhole_distortion must be [5] or [C,5] (k1 k2 p1 p2 k3 per camera; [4] / [C,4]: k3 = 0), got "
                         f"{tuple(np.shape(pinhole_distortion))}")
    if k.shape[1] == 4:
        k = np.concatenate([k, np.zeros((k.shape[0], 1))], axis=1)
    if not np.isfinite(k).all():
        raise ValueError("pinhole_distortion coefficients must be finite")
    return k if k.any() else None


def camera_model_id(camera_model, distortion=None, pinhole_distortion=None) -> int:
    """MGS_CAMERA_* of camera_model; with distortion= (lens_coefficients: valid only with "fisheye") that are not all
    zero, MGS_CAMERA_FISHEYE_KB; with pinhole_distortion= (pinhole_lens_coefficients: valid only with "pinhole") that are
    not all zero, MGS_CAMERA_PINHOLE_BC."""
    if camera_model not in CAMERA_MODELS:
        raise ValueError(f"camera_model {camera_model!r} not in {tuple(CAMERA_MODELS)}")
    if pinhole_distortion is not None:
        if distortion is not None:
            raise ValueError("pinhole_distortion= (the pinhole lens, k1 k2 p1 p2 k3) and distortion= (the fisheye lens, "
                             "k1..k4) are lenses of different camera models: give one of them")
        if camera_model != "pinhole":
            raise ValueError(f"pinhole_distortion= (OpenCV k1 k2 p1 p2 k3) needs camera_model='pinhole', got {camera_model!r}")
        return CAMERA_PINHOLE_BC if pinhole_lens_coefficients(pinhole_distortion) is not None else CAMERA_MODELS["pinhole"]
    if distortion is not None:
        if camera_model != "fisheye":
            raise ValueError(f"distortion= (fisheye lens coefficients k1..k4) needs camera_model='fisheye', got {camera_model!r}")
        if lens_coefficients(distortion) is not None:
            return CAMERA_FISHEYE_KB
    return CAMERA_MODELS[camera_model]


# (coefficient bytes, cameras, device) -> [C,7] device tensor k1..k4 | u_max | 0 0.  An entry is NEVER dropped: a captured
# graph (a Trainer step around rasterization(distortion=)) holds its address.  At _LENS_TAILS_MAX entries (28 bytes of
# payload each) further lenses are uploaded per call and owned by that call's rows alone.
_LENS_TAILS: dict = {}
_LENS_TAILS_MAX = 4096


def lens_rows(Ks: Tensor, distortion, pinhole_distortion=None) -> Tensor:
    """The [C,16] camera rows of MGS_CAMERA_FISHEYE_KB for Ks [C,3,3] on the device and a lens (lens_coefficients):
    K row-major | k1..k4 | u_max | 0 0, u_max = theta_max^2 computed per camera on the host in fp64
    (camera.lens_theta_max); with pinhole_distortion instead (pinhole_lens_coefficients) the rows of MGS_CAMERA_PINHOLE_BC:
    K | k1 k2 p1 p2 k3 | u_max | 0, u_max the radial fold (camera.pinhole_lens_u_max; FLT_MAX without one).  A LensRows
    hands its own rows back.  The lens part is uploaded once per distinct lens and
    device and kept for the life of the process, so a later call -- one under graph capture too -- only concatenates
    device tensors.  A lens this process has not seen cannot be uploaded under graph capture: ValueError (render once with it
    before capturing, as a warm-up does)."""
    from .camera import lens_theta_max, pinhole_lens_u_max
    C = Ks.shape[0]
    pinhole = pinhole_distortion is not None
    k = pinhole_lens_coefficients(pinhole_distortion, C) if pinhole else lens_coefficients(distortion, C)
    if k is None:
        raise ValueError("lens_rows needs distortion coefficients that are not all zero")
    if isinstance(k, LensRows):
        rows = k.rows
        require_device(rows)
        check_tensor("LensRows.rows", rows, torch.float32, (C, LENS_ROW_FLOATS), Ks.device)
        return rows
    key = (k.tobytes(), k.shape[0], Ks.device) + (("pinhole",) if pinhole else ())
    tail = _LENS_TAILS.get(key)
    if tail is None:
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("this lens has not been used in this process yet and its coefficients cannot be uploaded under "
                             "graph capture: render once with distortion= before capturing")
        host = np.zeros((k.shape[0], LENS_ROW_FLOATS - 9))
        host[:, :k.shape[1]] = k
        if pinhole:
            host[:, 5] = [min(pinhole_lens_u_max(row), float(np.finfo(np.float32).max)) for row in k]
        else:
            host[:, 4] = [lens_theta_max(row) ** 2 for row in k]
        tail = torch.from_numpy(host.astype(np.float32)).to(Ks.device)
        if len(_LENS_TAILS) < _LENS_TAILS_MAX:
            _LENS_TAILS[key] = tail
    return torch.cat([Ks.reshape(C, 9), tail.expand(C, -1)], dim=1).contiguous()


def radii_x(radii):
    """The per-Gaussian visibility / x-extent array of either radii layout: [N] (classic rule) or the planar [2,N]
    pair of per-axis extents the raw calls keep under the opacity-aware rule."""
    return radii if radii is None or radii.dim() == 1 else radii[0]


def radii_meta(radii):
    """Radii as the operator returns them: [N] (gsplat 1.4) or [N,2] (gsplat >= 1.5, per axis)."""
    return radii if radii is None or radii.dim() == 1 else radii.t()


def projection_fwd_raw(means, quats, scales, viewmat, K, width, height, eps2d, near_plane,
                       far_plane, radius_clip, calc_compensations, opacities=None, radius_rule=0, camera=0):
    """radius_rule 1 (MGS_RADIUS_OPACITY_AWARE): radii comes back planar [2,N] (x extents, y extents).
    camera: MGS_CAMERA_* (camera_model_id); under CAMERA_FISHEYE_KB / CAMERA_PINHOLE_BC `K` is the camera's 16-float row
    (lens_rows)."""
    n = means.shape[0]
    dev = means.device
    radii = torch.empty((2, n) if radius_rule else (n,), dtype=torch.int32, device=dev)
    means2d = torch.empty(n, 2, dtype=torch.float32, device=dev)
    depths = torch.empty(n, dtype=torch.float32, device=dev)
    conics = torch.empty(n, 3, dtype=torch.float32, device=dev)
    comp = torch.empty(n, dtype=torch.float32, device=dev) if calc_compensations else None
    check(_lib.lib().mgs_projection_fwd(n, ptr(means), ptr(quats), ptr(scales), ptr(viewmat),
                                        ptr(K), width, height, eps2d, near_plane, far_plane,
                                        radius_clip, ptr(radii_x(radii)), ptr(means2d), ptr(depths),
                                        ptr(conics), ptr(comp), ptr(opacities) if radius_rule else None,
                                        int(radius_rule), ptr(radii[1]) if radius_rule else None, int(camera),
                                        stream_handle()),
          "mgs_projection_fwd")
    return radii, means2d, depths, conics, comp


def project_color_fwd_raw(means, quats, scales, opacities, sh_degree, sh_coeffs, viewmat, K,
                          width, height, eps2d, near_plane, far_plane, radius_clip,
                          antialiased, with_depth, want_splats=False, bin_seed=None, lean=False, per_axis=False, camera=0,
                          raw=False):
    """Returns (radii, means2d, depths, conics, opac_aa|None, feats) and, with want_splats, a 7th
    item: the packed [N,12] records the raster kernels gather from.  bin_seed = "tight" | "classic":
    an 8th item (seed_info [N,2] i32, seed_sums [ceil(N/64)] i32) for isect_tiles_raw(seed=...).
    lean (needs want_splats and bin_seed): radii / means2d / conics / feats are not written and come back
    as None -- an inference frame, whose raster reads the records and whose binning reads the seed.
    per_axis: project with MGS_RADIUS_OPACITY_AWARE; radii is then planar [2,N] (radii_x / radii_meta).
    camera: the camera model, MGS_CAMERA_* (camera_model_id); under CAMERA_FISHEYE_KB / CAMERA_PINHOLE_BC `K` (and `Ks` of the frames
    calls below) holds 16-float camera rows (lens_rows).
    raw: scales are log-scales and opacities logits (MGS_PARAMS_RAW); every output is the activated form's.  Unless
    lean, the 5th item is then kept whether anti-aliased or not: the activated opacity (x compensation when
    anti-aliased), which the raster and project_color_bwd_raw need."""
    n = means.shape[0]
    dev = means.device
    if lean and not (want_splats and bin_seed is not None):
        raise ValueError("lean=True needs want_splats=True and a bin_seed")
    stride = 4 if with_depth else 3
    radii = means2d = conics = feats = None
    if not lean:
        radii = torch.empty((2, n) if per_axis else (n,), dtype=torch.int32, device=dev)
        means2d = torch.empty(n, 2, dtype=torch.float32, device=dev)
        conics = torch.empty(n, 3, dtype=torch.float32, device=dev)
        feats = torch.empty(n, stride, dtype=torch.float32, device=dev)
    depths = torch.empty(n, dtype=torch.float32, device=dev)
    keep_plain = bool(raw) and not antialiased and not lean
    opac = torch.empty(n, dtype=torch.float32, device=dev) if (antialiased or keep_plain) else None
    splats = torch.empty(n, 12, dtype=torch.float32, device=dev) if want_splats else None
    seed = None
    if bin_seed is not None and n > 0:
        seed = (torch.empty(n, 2, dtype=torch.int32, device=dev),
                torch.empty(max(1, -(-n // 64)), dtype=torch.int32, device=dev))
    check(_lib.lib().mgs_project_color_fwd(
        n, ptr(means), ptr(quats), ptr(scales), ptr(opacities), sh_degree, sh_coeffs.shape[1],
        ptr(sh_coeffs), ptr(viewmat), ptr(K), width, height, eps2d, near_plane, far_plane,
        radius_clip, ptr(radii_x(radii)), ptr(means2d), ptr(depths), ptr(conics), ptr(opac), stride,
        ptr(feats), ptr(splats),
        (BIN_TIGHT if bin_seed == "tight" else 0) | (BIN_RADIUS_OPACITY_AWARE if per_axis else 0) | camera_bin_flags(camera)
        | (PARAMS_RAW if raw else 0) | (PARAMS_OPAC_PLAIN if keep_plain else 0),
        ptr(seed[0]) if seed else None,
        ptr(seed[1]) if seed else None, ptr(radii[1]) if (per_axis and radii is not None) else None, stream_handle()),
        "mgs_project_color_fwd")
    out = (radii, means2d, depths, conics, opac, feats)
    if want_splats or bin_seed is not None:
        out = out + (splats,)
    if bin_seed is not None:
        out = out + (seed,)
    return out


def project_color_bwd_raw(means, quats, scales, opacities, sh_degree, sh_coeffs, viewmat, K, width, height, eps2d,
                          radii, conics, antialiased, feats, v_feats, v_means2d, v_conics, v_opac_aa, v_means, v_quats,
                          v_scales, v_sh, v_opacities, v_viewmat=None, accumulate=False, camera=0, v_depths=None, raw=False):
    """The chain rule of project_color_fwd_raw for one camera.  radii, conics, feats: what the forward returned;
    v_opac_aa: the cotangent of its opac_aa (antialiased only).  v_means / v_quats / v_scales / v_sh and, antialiased,
    v_opacities are overwritten, or added to with `accumulate`; v_viewmat [4,4] (optional) is always added to.
    raw (the forward's): scales / opacities are log-scales / logits; v_opac_aa -- the blend's opacity gradient -- and
    v_opacities are then needed anti-aliased or not, and v_scales / v_opacities are the gradients of the raw tensors.
    v_depths [N] (optional): a depth cotangent of its own, added to channel 3 of v_feats when feats is 4 wide and the only
    depth cotangent when it is 3 wide."""
    check(_lib.lib().mgs_project_color_bwd(
        means.shape[0], ptr(means), ptr(quats), ptr(scales), ptr(opacities), sh_degree, sh_coeffs.shape[1], ptr(sh_coeffs),
        ptr(viewmat), ptr(K), width, height, eps2d, ptr(radii_x(radii)), ptr(conics), int(antialiased), feats.shape[1],
        ptr(feats), ptr(v_feats), ptr(v_means2d), ptr(v_conics), ptr(v_depths), ptr(v_opac_aa), ptr(v_means), ptr(v_quats),
        ptr(v_scales), ptr(v_sh), ptr(v_opacities), ptr(v_viewmat), int(accumulate),
        int(camera) | (PARAMS_RAW if raw else 0), stream_handle()), "mgs_project_color_bwd")


class TileLists:
    """Depth-ordered per-tile lists of one camera (device resident, capacity sized)."""
    __slots__ = ("n_isect", "tile_ids", "flatten_ids", "tile_offsets", "tiles_per_gauss",
                 "isect_ids", "status", "capacity", "pair_info", "group_order", "splat_slots")


def _tag_splat_slots(tl: TileLists, splats) -> None:
    """mgs_isect_tiles(splat_slots=) writes the binning's record slots into words 10-11 of `splats` IN PLACE: the records
    belong to that binning from then on.  The tensor object and `tl` get the same new token; a later binning of the same
    object replaces the tensor's token, and no other tensor object carries one (_splat_slots_valid)."""
    tl.splat_slots = object()
    splats._mgs_splat_slots = tl.splat_slots


def isect_tiles_raw(means2d, radii, depths, tile_w, tile_h, capacity: int, cam_id=0, n_cams=1,
                    want_isect_ids=False, want_tiles_per_gauss=True,
                    want_pair_info=False, conics=None, opacities=None, seed=None,
                    want_tile_ids=True, want_group_order=True, splats=None) -> TileLists:
    """conics + opacities given: tile rectangles tightened to the tiles a Gaussian can reach with
    alpha >= 1/255 (shorter lists, bit-identical render); None: gsplat's classic rectangles.
    seed = (seed_info, seed_sums) from project_color_fwd_raw(bin_seed=...): the rectangles come from
    there (means2d / radii / conics / opacities are then not read and may be None; seed_sums is consumed).
    radii: [N], or planar [2,N] per-axis extents (gsplat >= 1.5's rule).
    splats (with want_pair_info): the packed records [N,12] of project_color_fwd_raw; the pairs' record slots are left in
    their padding words IN PLACE (include/mgs.h: splat_slots) -- the records are tied to this binning from then on -- and the
    lists remember which tensor object they annotated (_tag_splat_slots): rasterize_bwd_det_raw gathers nothing but the
    record while that pairing holds, and falls back to pair_info for any other tensor or once the records are binned again."""
    n = depths.shape[0]
    dev = depths.device
    out = TileLists()
    out.capacity = int(capacity)
    out.n_isect = torch.empty(1, dtype=torch.int32, device=dev)
    out.status = torch.empty(1, dtype=torch.int32, device=dev)       # written by every call
    out.tile_ids = torch.empty(capacity, dtype=torch.int32, device=dev) if want_tile_ids else None
    out.flatten_ids = torch.empty(capacity, dtype=torch.int32, device=dev)
    out.tile_offsets = torch.empty(tile_w * tile_h + 1, dtype=torch.int32, device=dev)
    out.tiles_per_gauss = (torch.empty(n, dtype=torch.int32, device=dev)
                           if want_tiles_per_gauss else None)
    out.isect_ids = torch.empty(capacity, dtype=torch.int64, device=dev) if want_isect_ids else None
    out.pair_info = torch.empty(n, 4, dtype=torch.int32, device=dev) if want_pair_info else None
    # launch order of the raster kernels' tiles (groups of four, longest lists first): a schedule, not a result
    out.group_order = (torch.empty((tile_w * tile_h + 3) // 4, dtype=torch.int32, device=dev) if want_group_order else None)
    annotate = splats is not None and want_pair_info
    args = [n, ptr(means2d), ptr(radii_x(radii)), ptr(radii[1]) if (radii is not None and radii.dim() == 2) else None,
            ptr(depths), ptr(conics), ptr(opacities), TILE_SIZE,
            tile_w, tile_h, cam_id, n_cams,
            capacity, ptr(out.tiles_per_gauss), ptr(out.n_isect), ptr(out.tile_ids),
            ptr(out.flatten_ids), ptr(out.isect_ids), ptr(out.tile_offsets), ptr(out.pair_info),
            ptr(out.group_order), ptr(out.status), ptr(seed[0]) if seed else None, ptr(seed[1]) if seed else None,
            ptr(splats) if annotate else None]
    out.splat_slots = False
    if annotate:
        _tag_splat_slots(out, splats)
    sized_call(_lib.lib().mgs_isect_tiles, args, dev, cached=True)
    return out


def _frames_call(means, quats, scales, opacities, sh_degree, sh_coeffs, viewmats, Ks, width, height, eps2d, near_plane,
                 far_plane, radius_clip, antialiased, with_depth, capacity, backgrounds, flags, out):
    """The frames mgs_render_frames / mgs_render_frames_train write (`out`, or new [C,H,W,ch] and [C,H,W] tensors) and
    the arguments both calls begin with."""
    dev = means.device
    C, ch = viewmats.shape[0], 4 if with_depth else 3
    if out is None:
        out = (torch.empty(C, height, width, ch, dtype=torch.float32, device=dev),
               torch.empty(C, height, width, dtype=torch.float32, device=dev))
    args = [means.shape[0], ptr(means), ptr(quats), ptr(scales), ptr(opacities), int(sh_degree), sh_coeffs.shape[1],
            ptr(sh_coeffs), C, ptr(viewmats), ptr(Ks), int(width), int(height), eps2d, near_plane, far_plane, radius_clip,
            int(bool(antialiased)), ch, flags, ptr(backgrounds), int(capacity)]
    return out[0], out[1], args


def render_frames_raw(means, quats, scales, opacities, sh_degree, sh_coeffs, viewmats, Ks, width, height,
                      eps2d, near_plane, far_plane, radius_clip, antialiased, with_depth, capacity,
                      backgrounds=None, expected_last=False, latency=False, out=None, tight=True, per_axis=False,
                      dataset=None, float_frame=True, camera=0, labels=None, raw=False):
    """mgs_render_frames: C inference frames in one C call (no per-Gaussian outputs, scratch reused from camera to
    camera).  viewmats [C,4,4], Ks [C,3,3], backgrounds [C,ch] or None.  Returns (render [C,H,W,ch], alphas [C,H,W],
    n_isects [C] i32, isect_status [C] i32); out = (render, alphas) to write into existing buffers.
    tight=False: gsplat's classic tile rectangles (MGS_FRAMES_CLASSIC_BOUNDS; same pixels, classic counts).
    dataset = (rgba uint8 [C,H,W,4], distance [C,H,W,1] or None, K): the dataset frames straight out of the raster
    (with_depth and expected_last required); float_frame=False then leaves render / alphas unwritten.
    raw: scales are log-scales and opacities logits (MGS_PARAMS_RAW).
    labels = (class_ids int32 [N], n_classes, labels uint8 [C,H,W], label_weights [C,H,W] or None): the call is
    mgs_render_frames_labeled, which also writes every camera's label frame (include/mgs_labels.h)."""
    dev = means.device
    C = viewmats.shape[0]
    render, alphas, args = _frames_call(means, quats, scales, opacities, sh_degree, sh_coeffs, viewmats, Ks, width, height,
                                        eps2d, near_plane, far_plane, radius_clip, antialiased, with_depth, capacity,
                                        backgrounds, frames_flags(expected_last, latency, tight, per_axis, camera, raw), out)
    n_isect = torch.empty(C, dtype=torch.int32, device=dev)
    status = torch.empty(C, dtype=torch.int32, device=dev)
    args += [ptr(render) if (float_frame or dataset is None) else None,
             ptr(alphas) if (float_frame or dataset is None) else None, ptr(n_isect), ptr(status)]
    ds = dataset_args(dataset, C, height, width, dev)
    args += list(ds[:4])
    if labels is not None:
        class_ids, n_classes, lab, lab_w = labels
        check_label_buffers(class_ids, means.shape[0], n_classes, lab, lab_w, (C, height, width))
        args += [ptr(class_ids), int(n_classes), ptr(lab), ptr(lab_w)]
        sized_call(_lib.lib().mgs_render_frames_labeled, args, dev, cached=True)
    else:
        sized_call(_lib.lib().mgs_render_frames, args, dev, cached=True)
    return render, alphas, n_isect, status


def checkpoint_buffer(capacity: int, tile_w: int, tile_h: int, channels: int, interval: int, device) -> Tensor:
    """The buffer rasterize_fwd_raw(checkpoints=...) writes for lists of up to `capacity` entries."""
    n = _lib.lib().mgs_raster_checkpoint_floats(int(capacity), tile_w, tile_h, channels, int(interval))
    if n == 0:
        raise ValueError(f"checkpoint interval {interval} is not a power of two >= 64")
    return torch.empty(n, dtype=torch.float32, device=device)


TRAIN_FIELDS = ("radii", "means2d", "depths", "conics", "opac_aa", "feats", "splats", "tiles_per_gauss", "pair_info",
                "tile_ids", "flatten_ids", "tile_offsets", "group_order", "last_ids", "checkpoints", "counts", "radii_y")


class TrainState:
    """Per-camera state of a batch of training frames (mgs_render_frames_train writes it, mgs_render_frames_backward
    reads it): one device buffer, fields at the offsets mgs_train_state_layout reports; `views(c)` hands them out as
    tensors without copying.  flags: the mgs_render_frames* flags word of the frames (the backward must get the forward's).
    raw: the frames are rendered from raw parameters (flags has PARAMS_RAW); the "opac_aa" field -- the opacity the raster
    saw -- is then kept whether anti-aliased or not."""

    def __init__(self, n, n_cams, width, height, channels, capacity, antialiased, interval, flags, device, raw=False):
        offs = (ctypes.c_size_t * len(TRAIN_FIELDS))()
        per = ctypes.c_size_t(0)
        self.raw = bool(raw)
        self.keep_opac = bool(antialiased) or self.raw
        check(_lib.lib().mgs_train_state_layout(n, width, height, channels, int(capacity), int(self.keep_opac), int(interval),
                                                offs, ctypes.byref(per)), "mgs_train_state_layout")
        self.offsets, self.per_camera = list(offs), per.value
        self.n, self.n_cams, self.width, self.height, self.channels = n, n_cams, width, height, channels
        self.capacity, self.antialiased, self.interval, self.flags = int(capacity), bool(antialiased), int(interval), flags
        self.buf = torch.empty(self.per_camera * n_cams + 256, dtype=torch.uint8, device=device)
        self.pad = (-self.buf.data_ptr()) % 256
        self.n_tiles = math.prod(tile_grid(width, height))

    def ptr(self) -> int:
        return self.buf.data_ptr() + self.pad

    def views(self, c: int) -> dict:
        n, cap, nt = self.n, self.capacity, self.n_tiles
        shapes = {"radii": (torch.int32, (n,)), "means2d": (torch.float32, (n, 2)), "depths": (torch.float32, (n,)),
                  "conics": (torch.float32, (n, 3)), "opac_aa": (torch.float32, (n,) if self.keep_opac else (0,)),
                  "feats": (torch.float32, (n, self.channels)), "splats": (torch.float32, (n, 12)),
                  "tiles_per_gauss": (torch.int32, (n,)), "pair_info": (torch.int32, (n, 4)), "tile_ids": (torch.int32, (cap,)),
                  "flatten_ids": (torch.int32, (cap,)), "tile_offsets": (torch.int32, (nt + 1,)),
                  "group_order": (torch.int32, ((nt + 3) // 4,)), "last_ids": (torch.int32, (self.height, self.width)),
                  "counts": (torch.int32, (2,)), "radii_y": (torch.int32, (n,))}
        out = {}
        base = self.pad + self.per_camera * c
        for name, off in zip(TRAIN_FIELDS, self.offsets):
            if name not in shapes:
                continue
            dt, shape = shapes[name]
            numel = 1
            for d_ in shape:
                numel *= d_
            nbytes = numel * (4)
            out[name] = self.buf[base + off:base + off + nbytes].view(dt).view(shape)
        return out

    def tile_lists(self, c: int, v: dict = None) -> "TileLists":
        v = v or self.views(c)
        tl = TileLists()
        tl.capacity = self.capacity
        tl.n_isect, tl.status = v["counts"][0:1], v["counts"][1:2]
        tl.tile_ids, tl.flatten_ids, tl.tile_offsets = v["tile_ids"], v["flatten_ids"], v["tile_offsets"]
        tl.tiles_per_gauss, tl.pair_info, tl.group_order, tl.isect_ids = v["tiles_per_gauss"], v["pair_info"], v["group_order"], None
        tl.splat_slots = True              # mgs_render_frames_train annotates the state's splat records
        return tl


def render_frames_train_raw(means, quats, scales, opacities, sh_degree, sh_coeffs, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radius_clip, antialiased, with_depth, capacity, interval,
                            backgrounds=None, expected_last=False, latency=True, tight=True, out=None, per_axis=False,
                            camera=0, raw=False):
    """mgs_render_frames_train: C training frames in one C call.  Returns (render [C,H,W,ch], alphas [C,H,W], TrainState).
    raw: scales are log-scales and opacities logits (MGS_PARAMS_RAW; the state remembers it for the backward)."""
    flags = frames_flags(expected_last, latency, tight, per_axis, camera, raw)
    render, alphas, args = _frames_call(means, quats, scales, opacities, sh_degree, sh_coeffs, viewmats, Ks, width, height,
                                        eps2d, near_plane, far_plane, radius_clip, antialiased, with_depth, capacity,
                                        backgrounds, flags, out)
    st = TrainState(means.shape[0], viewmats.shape[0], width, height, 4 if with_depth else 3, capacity, antialiased, interval,
                    flags, means.device, raw=raw)
    args += [int(interval), ptr(render), ptr(alphas), st.ptr()]
    sized_call(_lib.lib().mgs_render_frames_train, args, means.device, cached=True)
    return render, alphas, st


def render_frames_backward_raw(means, quats, scales, opacities, sh_degree, sh_coeffs, viewmats, Ks, eps2d, backgrounds, st,
                               render, alphas, v_render, v_alphas, absgrad=False, want_viewmats=False, raw=False):
    """mgs_render_frames_backward on a TrainState.  Returns (v_means, v_quats, v_scales, v_sh, v_opacities, v_viewmats|None,
    v_means2d [C,N,2], v_means2d_abs [C,N,2]|None).  raw must be the forward's (it travels in st.flags; the keyword is
    checked against it): v_scales / v_opacities are then the gradients of the log-scales / logits."""
    if bool(raw) != bool(st.flags & PARAMS_RAW):
        raise ValueError(f"raw={bool(raw)} but the TrainState was rendered with raw={bool(st.flags & PARAMS_RAW)}")
    dev = means.device
    C, n = viewmats.shape[0], means.shape[0]
    v_means, v_quats, v_scales = torch.empty_like(means), torch.empty_like(quats), torch.empty_like(scales)
    v_sh, v_opac = torch.empty_like(sh_coeffs), torch.empty_like(opacities)
    v_vm = torch.zeros_like(viewmats) if want_viewmats else None
    v_m2d = torch.empty(C, n, 2, dtype=torch.float32, device=dev)
    v_abs = torch.empty(C, n, 2, dtype=torch.float32, device=dev) if absgrad else None
    args = [n, ptr(means), ptr(quats), ptr(scales), ptr(opacities), int(sh_degree), sh_coeffs.shape[1], ptr(sh_coeffs), C,
            ptr(viewmats), ptr(Ks), st.width, st.height, eps2d, int(st.antialiased), st.channels, st.flags, ptr(backgrounds),
            st.capacity, st.interval, ptr(render), ptr(alphas), ptr(v_render), ptr(v_alphas), st.ptr(), ptr(v_means),
            ptr(v_quats), ptr(v_scales), ptr(v_sh), ptr(v_opac), ptr(v_vm), ptr(v_m2d), ptr(v_abs)]
    sized_call(_lib.lib().mgs_render_frames_backward, args, dev, cached=False)
    return v_means, v_quats, v_scales, v_sh, v_opac, v_vm, v_m2d, v_abs


def dataset_args(dataset, n_frames=None, height=None, width=None, device=None):
    """(ds_rgba, ds_distance, ds_distance_type, ds_Kinv_host, keep-alive) for the C calls that take a dataset output;
    dataset = (rgba uint8 [..,H,W,4], distance [..,H,W,1] or None, K [3,3]) or None.  The kernels write
    n_frames * height * width * 4 bytes of RGBA and as many distances through raw pointers: the buffers must hold exactly
    that, on the device the frame is rendered on (checked here; one K serves every camera of the call -- the
    intrinsics a dataset's cameras share)."""
    if dataset is None:
        return None, None, 0, None, None
    import numpy as np
    rgba, dist, K = dataset
    if rgba.dtype != torch.uint8 or not rgba.is_contiguous():
        raise ValueError("dataset rgba must be a contiguous uint8 tensor [..., H, W, 4]")
    if dist is not None and (not dist.is_contiguous() or dist.dtype not in (torch.float16, torch.float32, torch.float64)):
        raise ValueError("dataset distance must be a contiguous float16 / float32 / float64 tensor [..., H, W, 1]")
    require_device(rgba, dist)
    if device is not None and any(x is not None and x.device != device for x in (rgba, dist)):
        raise ValueError(f"dataset buffers must live on {device}, the device the frame is rendered on")
    if n_frames is not None:
        n_px = int(n_frames) * int(height) * int(width)
        if rgba.numel() != n_px * 4:
            raise ValueError(f"dataset rgba holds {rgba.numel()} bytes, {n_frames} frame(s) of {width}x{height} need {n_px * 4} "
                             f"([{n_frames},{height},{width},4] uint8)")
        if dist is not None and dist.numel() != n_px:
            raise ValueError(f"dataset distance holds {dist.numel()} values, {n_frames} frame(s) of {width}x{height} need {n_px} "
                             f"([{n_frames},{height},{width},1])")
    if dist is not None and K is None:
        raise ValueError("a dataset distance plane needs K (the 3x3 intrinsics the cameras of the call share)")
    kinv = np.ascontiguousarray(np.linalg.inv(np.asarray(K, dtype=np.float64).reshape(3, 3))) if dist is not None else None
    dtype_id = {torch.float64: 1, torch.float16: 2}.get(dist.dtype, 0) if dist is not None else 0
    return ptr(rgba), ptr(dist), dtype_id, (kinv.ctypes.data if kinv is not None else None), kinv


def rasterize_fwd_raw(means2d, conics, feats, opacities, background, width, height, tile_w,
                      tile_h, tile_offsets, flatten_ids, out=None, track_last=True, splats=None,
                      expected_last=False, latency=False, group_order=None, channels=None,
                      checkpoints=None, checkpoint_interval=0, dataset=None):
    """out = (render, alphas, last_ids|None) to write into existing buffers.
    dataset = (rgba uint8 [H,W,4], distance [H,W,1] f16 / f32 / f64 or None, K 3x3 numpy): the dataset frame straight
    out of the raster (include/mgs.h: ds_* arguments; 4 channels, expected_last, inference); out = (None, None, None)
    then skips the float frame altogether.  With `splats` (<= 4 channels)
    means2d / conics / feats / opacities are not read and may be None; give `channels` then.  track_last=False (or
    last_ids None) is the inference variant: no last_ids, one select less per pair.
    expected_last: the last channel leaves divided by max(alpha, 1e-10) ("ED" modes).
    latency: MGS_RASTER_LATENCY -- one wave per 8x8 block; faster when the launch has the GPU to itself
    (a single frame, a training step), slower in total work when several frames are in flight.
    group_order: TileLists.group_order -- the tiles are then started longest lists first.
    checkpoints (checkpoint_buffer(...)) + checkpoint_interval: the training variant also stores every pixel's state
    every `checkpoint_interval` list entries, for rasterize_bwd_det_raw(checkpoints=...)."""
    src = means2d if means2d is not None else splats
    n = src.shape[0]
    ch = int(channels) if channels is not None else feats.shape[-1]
    dev = src.device
    if out is None:
        render = torch.empty(height, width, ch, dtype=torch.float32, device=dev)
        alphas = torch.empty(height, width, dtype=torch.float32, device=dev)
        last_ids = (torch.empty(height, width, dtype=torch.int32, device=dev) if track_last
                    else None)
    else:
        render, alphas, last_ids = out
    ds = dataset_args(dataset, 1, height, width, dev)
    check(_lib.lib().mgs_rasterize_fwd(n, ptr(means2d), ptr(conics), ptr(feats), ptr(opacities),
                                       ptr(splats), ptr(background), ch, width, height, tile_w, tile_h,
                                       ptr(tile_offsets), ptr(flatten_ids), ptr(group_order),
                                       (RASTER_EXPECTED_LAST if expected_last else 0) | (RASTER_LATENCY if latency else 0),
                                       ptr(render), ptr(alphas), ptr(last_ids), ptr(checkpoints),
                                       int(checkpoint_interval), *ds[:4], stream_handle()),
          "mgs_rasterize_fwd")
    return render, alphas, last_ids


def class_ids_i32(class_ids, n: int) -> Tensor:
    """class_ids as the kernels read them: any integer tensor [n] on the device -> contiguous int32."""
    require_device(class_ids)
    if class_ids.dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.bool) or class_ids.is_complex():
        raise ValueError(f"class_ids must be an integer tensor, got {class_ids.dtype}")
    if tuple(class_ids.shape) != (n,):
        raise ValueError(f"class_ids shape {tuple(class_ids.shape)} != ({n},): one class per Gaussian")
    return class_ids.to(torch.int32).contiguous()


def check_n_classes(n_classes) -> int:
    n_classes = int(n_classes)
    if not 1 <= n_classes <= _lib.LABELS_MAX_CLASSES:
        raise ValueError(f"n_classes {n_classes} outside 1..{_lib.LABELS_MAX_CLASSES}")
    return n_classes


def check_label_buffers(class_ids, n, n_classes, labels, weights, shape) -> None:
    """The kernels write prod(shape) label bytes (and as many floats) through raw pointers and gather class_ids at every
    listed Gaussian: the buffers must hold exactly that."""
    check_n_classes(n_classes)
    check_tensor("class_ids", class_ids, torch.int32, (n,))
    check_tensor("labels", labels, torch.uint8, shape)
    if weights is not None:
        check_tensor("label_weights", weights, torch.float32, shape)
    require_device(class_ids, labels, weights)


def _walk_source(what: str, means2d, conics, opacities, splats):
    """The Gaussians a walk kernel gathers, through raw pointers: the packed records `splats` [n,12], or means2d [n,2],
    conics [n,3] and opacities [n].  Returns (n, device)."""
    src = splats if splats is not None else means2d
    if src is None or (splats is None and (conics is None or opacities is None)):
        raise ValueError(f"{what} needs splats, or means2d, conics and opacities")
    n = src.shape[0]
    if splats is not None:
        check_tensor("splats", splats, torch.float32, (n, 12))
    else:
        check_tensor("means2d", means2d, torch.float32, (n, 2))
        check_tensor("conics", conics, torch.float32, (n, 3))
        check_tensor("opacities", opacities, torch.float32, (n,))
    require_device(src, conics, opacities)
    return n, src.device


def _walk_lists(tl: "TileLists", width, height, use_group_order, tile_offsets):
    """The lists a walk kernel reads, through raw pointers, for a width x height frame: ((tile_w, tile_h), the offset table
    -- tile_offsets, or tl.tile_offsets where that is None --, tl.flatten_ids, tl.group_order or None).  Int32, contiguous
    and on the device, an offset per tile and the end of the last list, or a ValueError."""
    tile_w, tile_h = tile_grid(width, height)
    offsets = tile_offsets if tile_offsets is not None else tl.tile_offsets
    order = getattr(tl, "group_order", None) if use_group_order else None
    check_tensor("flatten_ids", tl.flatten_ids, torch.int32, (-1,))
    check_tensor("tile_offsets", offsets, torch.int32, (-1,))
    if order is not None:
        check_tensor("group_order", order, torch.int32, (-1,))
    if offsets.numel() < tile_w * tile_h + 1:
        raise ValueError(f"tile_offsets holds {offsets.numel()} entries, the frame has {tile_w * tile_h} tiles (+ 1)")
    require_device(tl.flatten_ids, offsets, order)
    return (tile_w, tile_h), offsets, tl.flatten_ids, order


def raster_labels_raw(tl: "TileLists", class_ids, n_classes, width, height, means2d=None, conics=None, opacities=None,
                      splats=None, out=None, return_weights=True, use_group_order=True, tile_offsets=None):
    """mgs_raster_labels on one camera's lists: labels uint8 [H,W] and (return_weights) label_weights [H,W], the class
    with the largest share of each pixel's blend weights and that share (include/mgs_labels.h).  class_ids: int32 [n]
    (class_ids_i32), n the rows of `splats` -- the packed records the frame's raster read -- or of means2d / conics /
    opacities.  out = (labels, label_weights|None) to write into existing buffers.  use_group_order: start the tiles in
    tl.group_order where the lists have one (a schedule, never a result); tile_offsets: another offset table than
    tl.tile_offsets (a camera's slice of a concatenated one)."""
    n, dev = _walk_source("raster_labels_raw", means2d, conics, opacities, splats)
    if out is None:
        labels = torch.empty(height, width, dtype=torch.uint8, device=dev)
        weights = torch.empty(height, width, dtype=torch.float32, device=dev) if return_weights else None
    else:
        labels, weights = out
    check_label_buffers(class_ids, n, n_classes, labels, weights, (height, width))
    (tile_w, tile_h), offsets, flatten_ids, order = _walk_lists(tl, width, height, use_group_order, tile_offsets)
    check(_lib.lib().mgs_raster_labels(n, ptr(means2d), ptr(conics), ptr(opacities), ptr(splats), ptr(class_ids),
                                       int(n_classes), width, height, tile_w, tile_h, ptr(offsets), ptr(flatten_ids),
                                       ptr(order), ptr(labels), ptr(weights), stream_handle()), "mgs_raster_labels")
    return labels, weights


def backdrop_f32(backdrop, dev) -> Optional[Tensor]:
    """backdrop as the kernels read it: None, or three floats on the device."""
    if backdrop is None:
        return None
    b = torch.as_tensor(backdrop, dtype=torch.float32, device=dev).contiguous()
    if tuple(b.shape) != (3,):
        raise ValueError(f"backdrop shape {tuple(b.shape)} != (3,)")
    return b


def raster_over_opaque_raw(tl: "TileLists", means2d, conics, opacities, feats, depths, fg_rgb, fg_depth, render, alphas,
                           width, height, backdrop=None, out=None, return_visibility=True, use_group_order=True,
                           tile_offsets=None):
    """mgs_raster_over_opaque on one camera's lists (include/mgs_hybrid.h): the frame's own blend stopped per pixel at
    the foreground's depth.  means2d [n,2], conics [n,3], opacities [n] (what the raster saw), feats [n,D] with rgb in the
    first three columns (D >= 3), depths [n]; fg_rgb [H,W,3], fg_depth [H,W]; render [H,W,4] ("RGB+ED"), alphas [H,W];
    backdrop None or a float32 tensor [3] on the device.  Returns (rgb [H,W,3], depth [H,W], fg_visibility [H,W] | None);
    out = the same triple to write into existing buffers.  use_group_order / tile_offsets: as raster_labels_raw."""
    n, dev = means2d.shape[0], means2d.device
    if feats.dim() != 2 or feats.shape[1] < 3:
        raise ValueError(f"feats shape {tuple(feats.shape)}: rgb in the first three of at least three columns")
    require_device(means2d)
    for name, t, shape in (("means2d", means2d, (n, 2)), ("conics", conics, (n, 3)), ("opacities", opacities, (n,)),
                           ("feats", feats, (n, -1)), ("depths", depths, (n,)),
                           ("fg_rgb", fg_rgb, (height, width, 3)), ("fg_depth", fg_depth, (height, width)),
                           ("render", render, (height, width, 4)), ("alphas", alphas, (height, width))):
        check_tensor(name, t, torch.float32, shape, dev)
    if backdrop is not None:
        check_tensor("backdrop", backdrop, torch.float32, (3,), dev)
    if out is None:
        rgb = torch.empty(height, width, 3, dtype=torch.float32, device=dev)
        depth = torch.empty(height, width, dtype=torch.float32, device=dev)
        vis = torch.empty(height, width, dtype=torch.float32, device=dev) if return_visibility else None
    else:
        rgb, depth, vis = out
        check_tensor("out rgb", rgb, torch.float32, (height, width, 3), dev)
        check_tensor("out depth", depth, torch.float32, (height, width), dev)
        if vis is not None:
            check_tensor("fg_visibility", vis, torch.float32, (height, width), dev)
    (tile_w, tile_h), offsets, flatten_ids, order = _walk_lists(tl, width, height, use_group_order, tile_offsets)
    check(_lib.lib().mgs_raster_over_opaque(
        n, ptr(means2d), ptr(conics), ptr(opacities), ptr(feats), int(feats.shape[1]), ptr(depths), ptr(fg_rgb),
        ptr(fg_depth), ptr(render), ptr(alphas), ptr(backdrop), width, height, tile_w, tile_h, ptr(offsets),
        ptr(flatten_ids), ptr(order), ptr(rgb), ptr(depth), ptr(vis), stream_handle()), "mgs_raster_over_opaque")
    return rgb, depth, vis


VOTE_ONE = 1 << 32       # a vote of one pixel at full weight (include/mgs_lift.h: unsigned Q32 fixed point)


def raster_votes_raw(tl: "TileLists", mask, n_classes, width, height, votes, means2d=None, conics=None, opacities=None,
                     splats=None, row_offset=0, use_group_order=True, tile_offsets=None):
    """mgs_raster_votes on one camera's lists: ADDS into votes int64 [rows, n_classes] (Q32 fixed point, votes_to_float)
    the blend weight every listed Gaussian contributes to the pixels of each class of `mask`, uint8 [H,W] with values
    outside 0..n_classes-1 (255, say) voting for nothing (include/mgs_lift.h).  The Gaussians are the rows of `splats` --
    the packed records the frame's raster read -- or of means2d / conics / opacities; list id `id` votes into row
    id - row_offset and nowhere if that is outside the buffer.  use_group_order / tile_offsets: as raster_labels_raw.
    Returns votes."""
    n, _ = _walk_source("raster_votes_raw", means2d, conics, opacities, splats)
    # the kernel gathers width * height mask bytes and adds into votes[row * n_classes + class]; torch's int64 carries the
    # unsigned Q32 value (it cannot wrap while views x pixels covered per view stays below 2^31: include/mgs_lift.h)
    n_classes = check_n_classes(n_classes)
    check_tensor("mask", mask, torch.uint8, (height, width))
    check_tensor("votes", votes, torch.int64, (-1, n_classes))
    require_device(mask, votes)
    (tile_w, tile_h), offsets, flatten_ids, order = _walk_lists(tl, width, height, use_group_order, tile_offsets)
    check(_lib.lib().mgs_raster_votes(n, ptr(means2d), ptr(conics), ptr(opacities), ptr(splats), ptr(mask), int(n_classes),
                                      width, height, tile_w, tile_h, ptr(offsets), ptr(flatten_ids), ptr(order),
                                      int(row_offset), votes.shape[0], ptr(votes), stream_handle()), "mgs_raster_votes")
    return votes


def assign_classes(votes: Tensor, min_vote: float = 0.0, out=None) -> Tuple[Tensor, Tensor]:
    """votes int64 [N,K] (rasterize_votes) -> (class_ids int32 [N], confidence float32 [N]): the class with the most
    votes, ties to the lowest class, if that vote exceeds min_vote (in pixels of full weight, >= 0), else -1; confidence is
    that vote's share of the row's total, 0 where the class is -1.  A Gaussian no mask pixel saw has class -1.
    out = (class_ids, confidence) to write into existing buffers.  No read-back: capturable in a graph."""
    require_device(votes)
    check_tensor("votes", votes, torch.int64, (-1, -1))
    n, k = votes.shape
    check_n_classes(k)
    if out is None:
        class_ids = torch.empty(n, dtype=torch.int32, device=votes.device)
        confidence = torch.empty(n, dtype=torch.float32, device=votes.device)
    else:
        class_ids, confidence = out
        require_device(class_ids, confidence)
        check_tensor("class_ids", class_ids, torch.int32, (n,))
        check_tensor("confidence", confidence, torch.float32, (n,))
    check(_lib.lib().mgs_lift_assign(n, k, ptr(votes), float(min_vote), ptr(class_ids), ptr(confidence), stream_handle()),
          "mgs_lift_assign")
    return class_ids, confidence


def votes_to_float(votes: Tensor) -> Tensor:
    """Q32 votes -> float64, in pixels of full weight."""
    return votes.to(torch.float64) * (1.0 / VOTE_ONE)


def rasterize_bwd_raw(means2d, conics, feats, opacities, background, width, height, tile_w,
                      tile_h, tile_offsets, flatten_ids, alphas, last_ids, v_render, v_alphas,
                      absgrad=False, accum=None):
    """Returns (v_means2d, v_conics, v_feats, v_opacities, v_means2d_abs|None).  `accum`
    supplies pre-zeroed / partially accumulated output buffers (float atomics add into them)."""
    n = means2d.shape[0]
    ch = feats.shape[-1]
    dev = means2d.device
    if accum is None:
        v_means2d = torch.zeros(n, 2, dtype=torch.float32, device=dev)
        v_conics = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        v_feats = torch.zeros(n, ch, dtype=torch.float32, device=dev)
        v_opac = torch.zeros(n, dtype=torch.float32, device=dev)
        v_abs = torch.zeros(n, 2, dtype=torch.float32, device=dev) if absgrad else None
    else:
        v_means2d, v_conics, v_feats, v_opac, v_abs = accum
    check(_lib.lib().mgs_rasterize_bwd(
        n, ptr(means2d), ptr(conics), ptr(feats), ptr(opacities), ptr(background), ch, width,
        height, tile_w, tile_h, ptr(tile_offsets), ptr(flatten_ids), ptr(alphas), ptr(last_ids),
        ptr(v_render), ptr(v_alphas), ptr(v_means2d), ptr(v_abs), ptr(v_conics), ptr(v_feats),
        ptr(v_opac), stream_handle()), "mgs_rasterize_bwd")
    return v_means2d, v_conics, v_feats, v_opac, v_abs


def _splat_slots_valid(tl, splats) -> bool:
    """The records `splats` carry the record slots of the binning that made `tl` (_tag_splat_slots): True for the
    train-state lists (mgs_render_frames_train annotates its own state), else only when `splats` is the very tensor
    object that binning annotated and no later binning has annotated it again."""
    tag = getattr(tl, "splat_slots", False)
    if splats is None or not tag:
        return False
    return tag is True or getattr(splats, "_mgs_splat_slots", None) is tag


def _record_floats(channels: int, absgrad: bool) -> int:
    """Floats per record of mgs_rasterize_bwd_det (include/mgs.h): 6 moments + padded channels (+2 with absgrad), rounded
    up to a multiple of 4.  Channels are padded to themselves up to 4, then to 8, 16, 32."""
    ch = int(channels)
    padded = ch if ch <= 4 else 8 if ch <= 8 else 16 if ch <= 16 else 32
    return (6 + padded + (2 if absgrad else 0) + 3) // 4 * 4


def rasterize_bwd_det_workspace_bytes(channels: int, absgrad: bool, capacity: int, tile_w: int, tile_h: int,
                                      checkpoint_interval: int = 0) -> int:
    """Bytes mgs_rasterize_bwd_det asks for (its own size query: host arithmetic, no GPU work)."""
    nb = ctypes.c_size_t(0)
    d = 256          # a non-null pointer the size query never dereferences
    ck = d if checkpoint_interval else None
    check(_lib.lib().mgs_rasterize_bwd_det(0, *[None] * 6, int(channels), tile_w * TILE_SIZE, tile_h * TILE_SIZE, tile_w, tile_h,
                                           *[None] * 9, int(capacity), ck, ck, int(checkpoint_interval), 0, None,
                                           d if absgrad else None, None, None, None, None, ctypes.byref(nb), None),
          "mgs_rasterize_bwd_det(size query)")
    return nb.value


def rasterize_bwd_det_workspace_layout(channels: int, absgrad: bool, capacity: int, tile_w: int, tile_h: int,
                                       checkpoint_interval: int = 0) -> dict:
    """Byte offsets of the workspace fields, as include/mgs.h documents them for mgs_rasterize_bwd_det: records at 0, flags
    at the next multiple of 256, the 256-byte counter header, the order / unit-table field, the big-rectangle lists (up to
    4 channels).  `total` equals rasterize_bwd_det_workspace_bytes (tests/test_bwd_reduce_host.py pins that)."""
    def up(x):
        return (int(x) + 255) // 256 * 256
    cap, n_tiles = max(int(capacity), 1), tile_w * tile_h
    rf = _record_floats(channels, absgrad)
    shift = 0
    while (1 << shift) < checkpoint_interval:
        shift += 1
    units = (cap >> shift) + n_tiles + 1 if checkpoint_interval else 0
    tables = 256 + (units + 32 * n_tiles) * 16 if checkpoint_interval else 0
    out = {"capacity": cap, "record_floats": rf, "shift": shift, "units": units, "records": 0}
    out["flags"] = up(cap * rf * 4)
    out["counters"] = out["flags"] + up(cap)
    out["order"] = out["counters"] + 256
    out["big_items"] = out["order"] + up(max(n_tiles * 4, tables, 1))
    out["total"] = out["big_items"] + (up(64 * (cap // 256 + 1) * 4) if channels <= 4 else 0)
    return out


def _aligned_workspace(workspace: Tensor, need: int, device) -> Tensor:
    """The caller's workspace from its first 256-byte aligned byte on: at least `need` bytes, or a ValueError."""
    check_tensor("workspace", workspace, torch.uint8, (-1,), device)
    workspace, pad = aligned_workspace(workspace, need, device)
    if workspace.numel() < pad + need:
        raise ValueError(f"workspace: {workspace.numel()} bytes, the call needs {need} + {pad} of alignment slack")
    return workspace[pad:]


def rasterize_bwd_det_workspace_views(workspace: Tensor, channels: int, absgrad: bool, capacity: int, tile_w: int,
                                      tile_h: int, checkpoint_interval: int = 0) -> dict:
    """Views (no copies) of a workspace rasterize_bwd_det_raw(workspace=...) used: `records` [capacity, record_floats]
    float32 and `flags` [capacity] uint8 (non-zero: the slot's record was written); `counters` [64] uint32 (the big
    lists' fill); for a checkpointed call also the unit tables: `unit_counts` [64] uint32 ([0] whole segments, [1 + c]
    partial segments of class c), `unit_whole` [units, 4] and `unit_part` [32, n_tiles, 4] int32 rows
    {tile, segment, list start, end of the tile's walk}."""
    lay = rasterize_bwd_det_workspace_layout(channels, absgrad, capacity, tile_w, tile_h, checkpoint_interval)
    w = _aligned_workspace(workspace, lay["total"], workspace.device)
    cap, rf, n_tiles = lay["capacity"], lay["record_floats"], tile_w * tile_h
    v = {"records": w[:cap * rf * 4].view(torch.float32).view(cap, rf),
         "flags": w[lay["flags"]:lay["flags"] + cap],
         "counters": w[lay["counters"]:lay["counters"] + 256].view(torch.int32)}
    if checkpoint_interval and channels <= 4:
        o, units = lay["order"], lay["units"]
        v["unit_counts"] = w[o:o + 256].view(torch.int32)
        v["unit_whole"] = w[o + 256:o + 256 + units * 16].view(torch.int32).view(units, 4)
        p = o + 256 + units * 16
        v["unit_part"] = w[p:p + 32 * n_tiles * 16].view(torch.int32).view(32, n_tiles, 4)
    return v


def _check_bwd_out(out, n: int, ch: int, absgrad: bool, dev):
    if len(out) != 5:
        raise ValueError("out: (v_means2d, v_conics, v_feats, v_opacities, v_means2d_abs|None)")
    if (out[4] is None) != (not absgrad):
        raise ValueError("out: v_means2d_abs is given exactly when absgrad is set")
    shapes = ((n, 2), (n, 3), (n, ch), (n,), (n, 2))
    names = ("v_means2d", "v_conics", "v_feats", "v_opacities", "v_means2d_abs")
    for t, shape, name in zip(out[:5 if absgrad else 4], shapes, names):
        check_tensor(f"out {name}", t, torch.float32, shape, dev)
    return tuple(out)


def rasterize_bwd_det_raw(means2d, conics, feats, opacities, background, width, height, tile_w,
                          tile_h, tl: "TileLists", alphas, last_ids, v_render, v_alphas,
                          absgrad=False, splats=None, canary_bytes=0, expected_render=None,
                          render_out=None, checkpoints=None, checkpoint_interval=0, records_only=False,
                          out=None, workspace=None):
    """Atomic-free, bit-reproducible raster backward (needs tl.pair_info from the binning).
    Returns freshly written (v_means2d, v_conics, v_feats, v_opacities, v_means2d_abs|None).
    expected_render: the forward's frame when it ran with expected_last (the kernel undoes the divide).
    checkpoints + checkpoint_interval + render_out (the forward's frame): the segmented walk (include/mgs.h).
    records_only: stop after the raster kernel (MGS_RASTER_BWD_RECORDS_ONLY; the returned tensors are not written).
    canary_bytes (tests): that many 0xA5 bytes are kept behind the workspace the library asked for
    and returned as a sixth value, so a test can see that nothing was written past the workspace.
    out = (v_means2d, v_conics, v_feats, v_opacities, v_means2d_abs|None): the caller's buffers are written (and
    returned) instead of fresh ones -- pre-filled with a sentinel they show a row no path wrote.
    workspace: the caller's uint8 tensor of at least rasterize_bwd_det_workspace_bytes(...) + the slack to the next
    multiple of 256 of its address (+ canary_bytes); used as is and left alive, rasterize_bwd_det_workspace_views reads
    the records and flags out of it."""
    n = means2d.shape[0]
    ch = feats.shape[-1]
    dev = means2d.device
    if out is not None:
        v_means2d, v_conics, v_feats, v_opac, v_abs = _check_bwd_out(out, n, ch, absgrad, dev)
    else:
        v_means2d = torch.empty(n, 2, dtype=torch.float32, device=dev)
        v_conics = torch.empty(n, 3, dtype=torch.float32, device=dev)
        v_feats = torch.empty(n, ch, dtype=torch.float32, device=dev)
        v_opac = torch.empty(n, dtype=torch.float32, device=dev)
        v_abs = torch.empty(n, 2, dtype=torch.float32, device=dev) if absgrad else None
    args = [n, ptr(means2d), ptr(conics), ptr(feats), ptr(opacities), ptr(splats), ptr(background),
            ch, width, height, tile_w, tile_h, ptr(tl.tile_offsets), ptr(tl.flatten_ids), ptr(alphas),
            ptr(last_ids), ptr(v_render), ptr(v_alphas), ptr(expected_render), ptr(tl.pair_info),
            ptr(getattr(tl, "group_order", None)), tl.capacity,
            ptr(render_out), ptr(checkpoints), int(checkpoint_interval),
            (RASTER_BWD_RECORDS_ONLY if records_only else 0) | (RASTER_BWD_SPLAT_SLOTS if _splat_slots_valid(tl, splats) else 0),
            ptr(v_means2d), ptr(v_abs), ptr(v_conics), ptr(v_feats), ptr(v_opac)]
    if workspace is not None:
        fn, nbytes = _lib.lib().mgs_rasterize_bwd_det, ctypes.c_size_t(0)
        check(fn(*args, None, ctypes.byref(nbytes), None), "mgs_rasterize_bwd_det(size query)")
        size = nbytes.value
        w = _aligned_workspace(workspace, size + int(canary_bytes), dev)
        canary = w[size:size + canary_bytes].fill_(0xA5) if canary_bytes else None
        check(fn(*args, w.data_ptr(), ctypes.byref(nbytes), stream_handle()), "mgs_rasterize_bwd_det")
    else:
        canary = sized_call(_lib.lib().mgs_rasterize_bwd_det, args, dev, cached=False, canary_bytes=canary_bytes)
    if canary_bytes:
        return v_means2d, v_conics, v_feats, v_opac, v_abs, canary
    return v_means2d, v_conics, v_feats, v_opac, v_abs


# ======================================================================================
# gsplat-compatible operators (multi-camera, autograd)
# ======================================================================================
class _Projection(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane,
                far_plane, radius_clip, calc_compensations, opacities=None, radius_rule=0, camera=0):
        C = viewmats.shape[0]
        outs = [projection_fwd_raw(means, quats, scales, viewmats[c], Ks[c], width, height,
                                   eps2d, near_plane, far_plane, radius_clip,
                                   calc_compensations, opacities, radius_rule, camera) for c in range(C)]
        radii_out = torch.stack([radii_meta(o[0]) for o in outs])      # [C,N], or [C,N,2] under the per-axis rule
        radii = torch.stack([radii_x(o[0]) for o in outs])             # [C,N]: > 0 = visible (what the backward reads)
        means2d = torch.stack([o[1] for o in outs])
        depths = torch.stack([o[2] for o in outs])
        conics = torch.stack([o[3] for o in outs])
        comps = torch.stack([o[4] for o in outs]) if calc_compensations else None
        ctx.save_for_backward(means, quats, scales, viewmats, Ks, radii, conics, comps)
        ctx.dims = (width, height, eps2d, camera)
        ctx.mark_non_differentiable(radii_out)
        return radii_out, means2d, depths, conics, comps

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, v_comps):
        means, quats, scales, viewmats, Ks, radii, conics, comps = ctx.saved_tensors
        width, height, eps2d, camera = ctx.dims
        n, C = means.shape[0], viewmats.shape[0]
        v_means = torch.zeros_like(means)
        v_quats = torch.zeros_like(quats)
        v_scales = torch.zeros_like(scales)
        want_view = ctx.needs_input_grad[3]
        v_viewmats = torch.zeros_like(viewmats) if want_view else None
        v_means2d, v_depths, v_conics = _f32c(v_means2d), _f32c(v_depths), _f32c(v_conics)
        v_comps = _f32c(v_comps) if comps is not None else None
        for c in range(C):
            check(_lib.lib().mgs_projection_bwd(
                n, ptr(means), ptr(quats), ptr(scales), ptr(viewmats[c]), ptr(Ks[c]), width,
                height, eps2d, ptr(radii[c]), ptr(conics[c]),
                ptr(comps[c]) if comps is not None else None,
                ptr(v_means2d[c]), ptr(v_depths[c]), ptr(v_conics[c]),
                ptr(v_comps[c]) if v_comps is not None else None, ptr(v_means), ptr(v_quats),
                ptr(v_scales), ptr(v_viewmats[c]) if want_view else None, int(camera), stream_handle()),
                "mgs_projection_bwd")
        return (v_means, v_quats, v_scales, v_viewmats, None, None, None, None, None, None,
                None, None, None, None, None)


def fully_fused_projection(means: Tensor, covars: Optional[Tensor], quats: Tensor,
                           scales: Tensor, viewmats: Tensor, Ks: Tensor, width: int,
                           height: int, eps2d: float = 0.3, near_plane: float = 0.01,
                           far_plane: float = 1e10, radius_clip: float = 0.0,
                           packed: bool = False, sparse_grad: bool = False,
                           calc_compensations: bool = False, opacities: Optional[Tensor] = None,
                           radius_rule: str = "classic", camera_model: str = "pinhole", distortion=None,
                           pinhole_distortion=None
                           ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Optional[Tensor]]:
    """World -> screen EWA projection of N Gaussians for C cameras.
    Returns radii [C,N] i32, means2d [C,N,2], depths [C,N], conics [C,N,3],
    compensations [C,N] | None.
    radius_rule: "classic" (gsplat 1.4, SURVEY.md A.2 step 5: one radius ceil(3 sqrt(lambda_1))) or "opacity_aware"
    (gsplat >= 1.5, SURVEY.md A.4: per-axis extents min(3.33, sqrt(2 ln(255 opacity))) sqrt(Sigma_ii), radii [C,N,2];
    `opacities` [N] optional as in that operator, no gradient flows to it -- the extent is not differentiable).
    camera_model: "pinhole", "ortho" or "fisheye" (ideal equidistant, r = f theta), as gsplat's operator; include/mgs.h
    MGS_CAMERA_* gives the maps.  Depths are camera z under every model.
    distortion (with "fisheye"): OpenCV fisheye coefficients k1..k4, host data [4] or [C,4] -- theta_d = theta (1 + k1 theta^2
    + ... + k4 theta^8); Gaussians past the angle where that polynomial folds back are culled.  None / all zero: the ideal lens.
    pinhole_distortion (with "pinhole"): OpenCV's distCoeffs k1 k2 p1 p2 k3, host data [5] or [C,5] ([4]: k3 = 0) -- the
    radial / tangential lens of include/mgs_lens_pinhole.h with its three culls (rasterization's docstring).  None / all
    zero: the plain pinhole."""
    if covars is not None:
        raise NotImplementedError("precomputed covariances are not supported; pass quats+scales")
    if packed:
        raise NotImplementedError("packed=True is not supported (nerfstudio uses packed=False)")
    require_device(means, quats, scales, viewmats, Ks)
    means, quats, scales = _f32c(means), _f32c(quats), _f32c(scales)
    viewmats, Ks = _f32c(viewmats), _f32c(Ks)
    if means.dim() != 2 or means.shape[1] != 3 or quats.shape != (means.shape[0], 4) \
            or scales.shape != means.shape:
        raise ValueError("expected means [N,3], quats [N,4], scales [N,3]")
    if viewmats.dim() != 3 or viewmats.shape[1:] != (4, 4) or Ks.shape != (viewmats.shape[0], 3, 3):
        raise ValueError("expected viewmats [C,4,4], Ks [C,3,3]")
    rule = radius_rule_id(radius_rule)
    camera = camera_model_id(camera_model, distortion, pinhole_distortion)
    if camera in LENS_CAMERAS:
        Ks = lens_rows(Ks, distortion, pinhole_distortion)
    if opacities is not None:
        require_device(opacities)
        opacities = _f32c(opacities.detach())
        if opacities.shape != (means.shape[0],):
            raise ValueError("expected opacities [N]")
    return _Projection.apply(means, quats, scales, viewmats, Ks, int(width), int(height),
                             float(eps2d), float(near_plane), float(far_plane),
                             float(radius_clip), bool(calc_compensations), opacities if rule else None, rule, camera)


class _SphericalHarmonics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, degree, dirs, coeffs, masks):
        n = dirs.shape[0]
        colors = torch.empty(n, 3, dtype=torch.float32, device=dirs.device)
        check(_lib.lib().mgs_sh_fwd(n, degree, coeffs.shape[1], ptr(dirs), ptr(coeffs), ptr(masks),
                                    ptr(colors), stream_handle()), "mgs_sh_fwd")
        ctx.save_for_backward(dirs, coeffs, masks)
        ctx.degree = degree
        return colors

    @staticmethod
    def backward(ctx, v_colors):
        dirs, coeffs, masks = ctx.saved_tensors
        n = dirs.shape[0]
        v_coeffs = torch.empty_like(coeffs)
        v_dirs = torch.empty_like(dirs) if ctx.needs_input_grad[1] else None
        check(_lib.lib().mgs_sh_bwd(n, ctx.degree, coeffs.shape[1], ptr(dirs), ptr(coeffs),
                                    ptr(masks), ptr(_f32c(v_colors)), ptr(v_coeffs), ptr(v_dirs),
                                    stream_handle()), "mgs_sh_bwd")
        return None, v_dirs, v_coeffs, None


def spherical_harmonics(degrees_to_use: int, dirs: Tensor, coeffs: Tensor,
                        masks: Optional[Tensor] = None) -> Tensor:
    """colors[...,3] = sum_k Y_k(normalize(dirs)) coeffs[...,k,:] for k < (degrees_to_use+1)^2."""
    require_device(dirs, coeffs, masks)
    if not 0 <= degrees_to_use <= 3:
        raise ValueError(f"degrees_to_use={degrees_to_use} outside 0..3")
    if coeffs.shape[-2] < (degrees_to_use + 1) ** 2:
        raise ValueError("coeffs holds fewer than (degrees_to_use+1)^2 coefficients")
    if dirs.shape[:-1] != coeffs.shape[:-2] or dirs.shape[-1] != 3 or coeffs.shape[-1] != 3:
        raise ValueError("expected dirs [...,3] and coeffs [...,K,3] with equal batch dims")
    batch = dirs.shape[:-1]
    d = _f32c(dirs).reshape(-1, 3)
    c = _f32c(coeffs).reshape(-1, coeffs.shape[-2], 3)
    m = None
    if masks is not None:
        m = masks.reshape(-1).to(torch.uint8).contiguous()
    return _SphericalHarmonics.apply(int(degrees_to_use), d, c, m).reshape(*batch, 3)


@torch.no_grad()
def isect_tiles(means2d: Tensor, radii: Tensor, depths: Tensor, tile_size: int,
                tile_width: int, tile_height: int, sort: bool = True, packed: bool = False,
                n_cameras: Optional[int] = None, camera_ids: Optional[Tensor] = None,
                gaussian_ids: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Tile intersection + sort.  Returns tiles_per_gauss [C,N] i32, isect_ids [n_isects] i64
    (cam | tile | depth bits, ascending), flatten_ids [n_isects] i32 (cam*N + gaussian).
    radii [C,N] (one radius: the square mean +- radius) or [C,N,2] (per-axis extents, gsplat >= 1.5).
    Reads the intersection count back to size the outputs (one sync, as the reference
    operator does); the render path in rendering.py avoids that with a capacity."""
    if packed or not sort:
        raise NotImplementedError("only packed=False, sort=True is supported")
    if tile_size != TILE_SIZE:
        raise NotImplementedError(f"tile_size must be {TILE_SIZE}")
    require_device(means2d, radii, depths)
    C, N = means2d.shape[0], means2d.shape[1]
    means2d, depths = _f32c(means2d), _f32c(depths)
    radii = radii.to(torch.int32)
    if radii.dim() == 3:
        if radii.shape[-1] != 2:
            raise ValueError("expected radii [C,N] or [C,N,2]")
        radii = radii.transpose(1, 2)                # planar [C,2,N] for the raw call
    radii = radii.contiguous()
    tpg, keys, ids = [], [], []
    for c in range(C):
        cap = max(1, int(_upper_bound_isects(radii[c], tile_width, tile_height)))
        tl = isect_tiles_raw(means2d[c], radii[c], depths[c], tile_width, tile_height, cap, c, C,
                             want_isect_ids=True)
        n = int(tl.n_isect.item())
        tpg.append(tl.tiles_per_gauss)
        keys.append(tl.isect_ids[:n])
        ids.append(tl.flatten_ids[:n] + c * N if c else tl.flatten_ids[:n])
    return torch.stack(tpg), torch.cat(keys), torch.cat(ids)


def _upper_bound_isects(radii_c: Tensor, tile_w: int, tile_h: int) -> int:
    """Cheap device-side bound: sum over visible Gaussians of min((2r/16+2)^2, tiles); radii_c [N] or planar [2,N]."""
    rx = radii_x(radii_c).clamp_min(0).to(torch.float32)
    ry = rx if radii_c.dim() == 1 else radii_c[1].clamp_min(0).to(torch.float32)
    side_x = torch.floor(2.0 * rx / TILE_SIZE) + 2.0
    side_y = torch.floor(2.0 * ry / TILE_SIZE) + 2.0
    per = torch.minimum(side_x.clamp_max(tile_w) * side_y.clamp_max(tile_h),
                        torch.tensor(float(tile_w * tile_h), device=rx.device))
    return int(torch.where(radii_x(radii_c) > 0, per, torch.zeros_like(per)).sum().item())


@torch.no_grad()
def isect_offset_encode(isect_ids: Tensor, n_cameras: int, tile_width: int,
                        tile_height: int) -> Tensor:
    """First sorted index of every (camera, tile): int32 [C, tile_height, tile_width]."""
    require_device(isect_ids)
    isect_ids = isect_ids.contiguous()
    out = torch.empty(n_cameras, tile_height, tile_width, dtype=torch.int32,
                      device=isect_ids.device)
    check(_lib.lib().mgs_isect_offset_encode(isect_ids.numel(), ptr(isect_ids), n_cameras,
                                             tile_width, tile_height, ptr(out), stream_handle()),
          "mgs_isect_offset_encode")
    return out


def _gsplat_lists(isect_offsets: Tensor, flatten_ids: Tensor, C: int, width: int, height: int, tile_size: int, *arrays):
    """gsplat's lists -- isect_offsets [C,th,tw], flatten_ids [n_isects] with ids cam*N + gaussian -- as the raw calls
    read them: (tl, n_tiles) with tl.flatten_ids int32 and tl.tile_offsets the int32 table of all C cameras with the end
    of the last list appended; camera c walks tl with tile_offsets=tl.tile_offsets[c * n_tiles:] over the flat [C*N,...]
    arrays.  One conversion, one full and one cat per operator call.  The refusals come in the operators' order: the tile
    size, then a CPU tensor among the lists and `arrays` (the operator's other tensors), then the grid."""
    if tile_size != TILE_SIZE:
        raise NotImplementedError(f"tile_size must be {TILE_SIZE}")
    require_device(isect_offsets, flatten_ids, *arrays)
    tile_w, tile_h = tile_grid(width, height)
    if tuple(isect_offsets.shape) != (C, tile_h, tile_w):
        raise ValueError(f"isect_offsets shape {tuple(isect_offsets.shape)} != {(C, tile_h, tile_w)}")
    tl = TileLists()
    tl.flatten_ids = flatten_ids.to(torch.int32).contiguous()
    end = torch.full((1,), tl.flatten_ids.numel(), dtype=torch.int32, device=flatten_ids.device)
    tl.tile_offsets = torch.cat([isect_offsets.reshape(-1).to(torch.int32), end])
    return tl, tile_w * tile_h


def _flat_arrays(means2d: Tensor, conics: Tensor, opacities: Tensor):
    """The [C,N,...] arrays of a non-differentiable operator: (C, N, their detached float32 flat [C*N,...] views)."""
    C, N = means2d.shape[0], means2d.shape[1]
    if conics.shape != (C, N, 3) or opacities.shape != (C, N) or means2d.shape != (C, N, 2):
        raise ValueError("expected means2d [C,N,2], conics [C,N,3], opacities [C,N]")
    return C, N, (_f32c(means2d.detach()).view(C * N, 2), _f32c(conics.detach()).view(C * N, 3),
                  _f32c(opacities.detach()).view(C * N))


class _RasterizeToPixels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means2d, conics, colors, opacities, backgrounds, width, height,
                offsets_ext, flatten_ids, absgrad):
        C, N, ch = colors.shape
        tile_w, tile_h = tile_grid(width, height)
        n_tiles = tile_w * tile_h
        dev = means2d.device
        render = torch.empty(C, height, width, ch, dtype=torch.float32, device=dev)
        alphas = torch.empty(C, height, width, dtype=torch.float32, device=dev)
        last_ids = torch.empty(C, height, width, dtype=torch.int32, device=dev)
        for c in range(C):
            # ids in flatten_ids are cam*N + gaussian: hand the kernels the flat [C*N,...] views
            rasterize_fwd_raw(means2d.view(C * N, 2), conics.view(C * N, 3),
                              colors.view(C * N, ch), opacities.view(C * N),
                              backgrounds[c] if backgrounds is not None else None, width, height,
                              tile_w, tile_h, offsets_ext[c * n_tiles:], flatten_ids,
                              out=(render[c], alphas[c], last_ids[c]))
        ctx.save_for_backward(means2d, conics, colors, opacities, backgrounds, offsets_ext,
                              flatten_ids, alphas, last_ids)
        ctx.dims = (width, height, tile_w, tile_h, absgrad)
        return render, alphas.unsqueeze(-1)

    @staticmethod
    def backward(ctx, v_render, v_alphas):
        (means2d, conics, colors, opacities, backgrounds, offsets_ext, flatten_ids, alphas,
         last_ids) = ctx.saved_tensors
        width, height, tile_w, tile_h, absgrad = ctx.dims
        C, N, ch = colors.shape
        n_tiles = tile_w * tile_h
        dev = means2d.device
        v_render = _f32c(v_render)
        v_alphas = _f32c(v_alphas).reshape(C, height, width)
        acc = (torch.zeros(C * N, 2, device=dev), torch.zeros(C * N, 3, device=dev),
               torch.zeros(C * N, ch, device=dev), torch.zeros(C * N, device=dev),
               torch.zeros(C * N, 2, device=dev) if absgrad else None)
        for c in range(C):
            rasterize_bwd_raw(means2d.view(C * N, 2), conics.view(C * N, 3),
                              colors.view(C * N, ch), opacities.view(C * N),
                              backgrounds[c] if backgrounds is not None else None, width, height,
                              tile_w, tile_h, offsets_ext[c * n_tiles:], flatten_ids, alphas[c],
                              last_ids[c], v_render[c], v_alphas[c], absgrad, accum=acc)
        v_bg = None
        if backgrounds is not None and ctx.needs_input_grad[4]:
            v_bg = (v_render * (1.0 - alphas).unsqueeze(-1)).sum(dim=(1, 2))
        if absgrad:
            means2d.absgrad = acc[4].view(C, N, 2)
        return (acc[0].view(C, N, 2), acc[1].view(C, N, 3), acc[2].view(C, N, ch),
                acc[3].view(C, N), v_bg, None, None, None, None, None)


def rasterize_to_pixels(means2d: Tensor, conics: Tensor, colors: Tensor, opacities: Tensor,
                        image_width: int, image_height: int, tile_size: int,
                        isect_offsets: Tensor, flatten_ids: Tensor,
                        backgrounds: Optional[Tensor] = None, masks: Optional[Tensor] = None,
                        packed: bool = False, absgrad: bool = False) -> Tuple[Tensor, Tensor]:
    """Depth-ordered alpha compositing.  means2d [C,N,2], conics [C,N,3], colors [C,N,ch],
    opacities [C,N], isect_offsets [C,th,tw], flatten_ids [n_isects] ->
    render_colors [C,H,W,ch], render_alphas [C,H,W,1]."""
    if packed:
        raise NotImplementedError("packed=True is not supported")
    if masks is not None:
        raise NotImplementedError("tile masks are not supported")
    tl, _ = _gsplat_lists(isect_offsets, flatten_ids, means2d.shape[0], image_width, image_height, tile_size,
                          means2d, conics, colors, opacities, backgrounds)
    ch = colors.shape[-1]
    if not 1 <= ch <= 32:
        raise ValueError(f"{ch} colour channels: supported range is 1..32")
    return _RasterizeToPixels.apply(_f32c(means2d), _f32c(conics), _f32c(colors),
                                    _f32c(opacities), _f32c(backgrounds), int(image_width),
                                    int(image_height), tl.tile_offsets, tl.flatten_ids, bool(absgrad))


@torch.no_grad()
def rasterize_labels(means2d: Tensor, conics: Tensor, opacities: Tensor, class_ids: Tensor, n_classes: int,
                     image_width: int, image_height: int, tile_size: int, isect_offsets: Tensor, flatten_ids: Tensor,
                     return_weights: bool = False):
    """Per-pixel part labels of the frames rasterize_to_pixels blends from the same arguments: means2d [C,N,2], conics
    [C,N,3], opacities [C,N], class_ids [N] (any integer type), isect_offsets [C,th,tw], flatten_ids [n_isects] ->
    labels [C,H,W] uint8, the class k in 0..n_classes-1 (n_classes <= 32) with the largest sum of blend weights at the
    pixel, ties to the lowest k, 255 where no counted Gaussian has such a class; with return_weights also that sum,
    [C,H,W] float32.  A Gaussian whose class is outside 0..n_classes-1 occludes and is never reported.  The weights are
    the blend's own bit for bit.  Not differentiable."""
    width, height = int(image_width), int(image_height)
    tl, n_tiles = _gsplat_lists(isect_offsets, flatten_ids, means2d.shape[0], width, height, tile_size,
                                means2d, conics, opacities)
    C, N, flat = _flat_arrays(means2d, conics, opacities)
    n_classes = check_n_classes(n_classes)
    dev = means2d.device
    cls = class_ids_i32(class_ids, N).repeat(C)          # ids in flatten_ids are cam*N + gaussian: the classes once per camera
    labels = torch.empty(C, height, width, dtype=torch.uint8, device=dev)
    weights = torch.empty(C, height, width, dtype=torch.float32, device=dev) if return_weights else None
    for c in range(C):
        raster_labels_raw(tl, cls, n_classes, width, height, *flat, out=(labels[c], weights[c] if return_weights else None),
                          use_group_order=False, tile_offsets=tl.tile_offsets[c * n_tiles:])
    return (labels, weights) if return_weights else labels


@torch.no_grad()
def rasterize_over_opaque(means2d: Tensor, conics: Tensor, colors: Tensor, depths: Tensor, opacities: Tensor,
                          fg_rgb: Tensor, fg_depth: Tensor, render_colors: Tensor, render_alphas: Tensor,
                          image_width: int, image_height: int, tile_size: int, isect_offsets: Tensor, flatten_ids: Tensor,
                          backdrop=None, return_visibility: bool = False):
    """The exact composite of the frames rasterize_to_pixels blends from the same arguments with an opaque foreground
    (include/mgs_hybrid.h): each pixel's own front-to-back blend, stopped at the foreground's depth, the foreground
    entering at the transmittance reached there.  means2d [C,N,2], conics [C,N,3], colors [C,N,D] (rgb in the first three
    columns, D >= 3), depths [C,N], opacities [C,N]; fg_rgb [C,H,W,3], fg_depth [C,H,W] (z-depth, 0 where no face is:
    rasterize_mesh's outputs as they are); render_colors [C,H,W,4] in "RGB+ED" mode and render_alphas [C,H,W] or
    [C,H,W,1]: the plain frame, copied where there is no foreground (+ (1 - alpha) backdrop, depth +inf where alpha is 0);
    isect_offsets [C,th,tw], flatten_ids [n_isects]; backdrop None or three floats.
    Returns (rgb [C,H,W,3], depth [C,H,W]) and with return_visibility also fg_visibility [C,H,W], the share of the
    foreground that reaches the eye (0 where there is none).  Not differentiable."""
    width, height = int(image_width), int(image_height)
    tl, n_tiles = _gsplat_lists(isect_offsets, flatten_ids, means2d.shape[0], width, height, tile_size,
                                means2d, conics, colors, depths, opacities, fg_rgb, fg_depth, render_colors, render_alphas)
    C, N, flat = _flat_arrays(means2d, conics, opacities)
    if colors.dim() != 3 or colors.shape[:2] != (C, N) or colors.shape[2] < 3 or depths.shape != (C, N):
        raise ValueError("expected colors [C,N,D] with rgb in the first three of D >= 3 columns, and depths [C,N]")
    if tuple(fg_rgb.shape) != (C, height, width, 3) or tuple(fg_depth.shape) != (C, height, width):
        raise ValueError(f"expected fg_rgb {(C, height, width, 3)} and fg_depth {(C, height, width)}")
    if tuple(render_colors.shape) != (C, height, width, 4):
        raise ValueError(f"render_colors shape {tuple(render_colors.shape)} != {(C, height, width, 4)}: an 'RGB+ED' frame")
    if render_alphas.numel() != C * height * width or render_alphas.shape[:3] != (C, height, width):
        raise ValueError(f"render_alphas shape {tuple(render_alphas.shape)} is neither {(C, height, width)} nor "
                         f"{(C, height, width, 1)}")
    dev = means2d.device
    colors, depths = _f32c(colors.detach()).view(C * N, colors.shape[2]), _f32c(depths.detach()).view(C * N)
    fg_rgb, fg_depth = _f32c(fg_rgb.detach()), _f32c(fg_depth.detach())
    render = _f32c(render_colors.detach())
    alphas = _f32c(render_alphas.detach()).reshape(C, height, width)
    bd = backdrop_f32(backdrop, dev)
    rgb = torch.empty(C, height, width, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(C, height, width, dtype=torch.float32, device=dev)
    vis = torch.empty(C, height, width, dtype=torch.float32, device=dev) if return_visibility else None
    for c in range(C):
        raster_over_opaque_raw(tl, *flat, colors, depths, fg_rgb[c], fg_depth[c], render[c], alphas[c], width, height,
                               backdrop=bd, out=(rgb[c], depth[c], vis[c] if return_visibility else None),
                               use_group_order=False, tile_offsets=tl.tile_offsets[c * n_tiles:])
    return (rgb, depth, vis) if return_visibility else (rgb, depth)


@torch.no_grad()
def rasterize_votes(means2d: Tensor, conics: Tensor, opacities: Tensor, masks: Tensor, n_classes: int, image_width: int,
                    image_height: int, tile_size: int, isect_offsets: Tensor, flatten_ids: Tensor,
                    votes: Optional[Tensor] = None) -> Tensor:
    """2D part masks lifted onto the Gaussians of the frames rasterize_to_pixels blends from the same arguments: means2d
    [C,N,2], conics [C,N,3], opacities [C,N], masks [C,H,W] uint8 (a value outside 0..n_classes-1 votes for nothing),
    isect_offsets [C,th,tw], flatten_ids [n_isects] -> votes int64 [N, n_classes]: votes[i,k] is the sum over all C
    cameras and all pixels with mask == k of the weight the blend gives Gaussian i there, as unsigned Q32 fixed point
    (votes_to_float).  Integers: the same bits in every run and under any split of the cameras over calls; votes=
    continues an earlier call.  assign_classes turns them into class ids.  Not differentiable."""
    width, height = int(image_width), int(image_height)
    tl, n_tiles = _gsplat_lists(isect_offsets, flatten_ids, means2d.shape[0], width, height, tile_size,
                                means2d, conics, opacities, masks, votes)
    C, N, flat = _flat_arrays(means2d, conics, opacities)
    n_classes = check_n_classes(n_classes)
    if tuple(masks.shape) != (C, height, width) or masks.dtype != torch.uint8:
        raise ValueError(f"masks must be a uint8 tensor {(C, height, width)}")
    masks = masks.contiguous()
    if votes is None:
        votes = torch.zeros(N, n_classes, dtype=torch.int64, device=means2d.device)
    elif tuple(votes.shape) != (N, n_classes):
        raise ValueError(f"votes shape {tuple(votes.shape)} != {(N, n_classes)}")
    for c in range(C):       # ids in flatten_ids are cam*N + gaussian: camera c's votes go to rows id - c*N
        raster_votes_raw(tl, masks[c], n_classes, width, height, votes, *flat, row_offset=c * N, use_group_order=False,
                         tile_offsets=tl.tile_offsets[c * n_tiles:])
    return votes
