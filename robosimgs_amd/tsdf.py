"""From a Gaussian scene to a triangle mesh: depth frames fused into a truncated signed distance (TSDF) volume, and the
volume's isosurface (include/mgs_tsdf.h, csrc/tsdf.hip, csrc/tsdf_tets.h).

    vol = TSDFVolume.from_bounds(lo, hi, voxel_size=0.02)
    frames, alphas, _ = rasterization(..., render_mode="RGB+ED")        # [C,H,W,4], [C,H,W,1]
    vol.integrate(frames, viewmats, Ks, alphas=alphas)
    vol.extract_mesh().to_obj("background.obj")                          # what a simulator collides with

A dense grid of nx x ny x nz samples, x fastest; sample (i, j, k) sits at origin + (i + 0.5, j + 0.5, k + 0.5) voxel_size.  One
call of `integrate` is one launch for all its cameras and reads and writes the volume once; a sample's updates are applied
in camera order, so the volume holds the same bytes however the views are chunked into calls.  A `[C,H,W]` depth tensor
alone (a depth sensor's image) fuses without colour.  Plain pinhole cameras and z-depth only.  Everything here is eager.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import MgsError, check, check_tensor, ptr, require_device, stream_handle
from .mesh import Mesh


def _volume_struct(dims, origin, voxel_size, trunc, max_weight, tsdf, weight, color) -> _lib.TsdfVolume:
    return _lib.TsdfVolume(int(dims[0]), int(dims[1]), int(dims[2]), (ctypes.c_float * 3)(*[float(x) for x in origin]),
                           float(voxel_size), float(trunc), float(max_weight), ptr(tsdf), ptr(weight), ptr(color))


def _cameras(viewmats, Ks, C: int, device) -> Tuple[Tensor, Tensor]:
    viewmats = torch.as_tensor(viewmats, dtype=torch.float32, device=device).reshape(-1, 4, 4).contiguous()
    Ks = torch.as_tensor(Ks, dtype=torch.float32, device=device).reshape(-1, 3, 3).contiguous()
    check_tensor("viewmats", viewmats, torch.float32, (C, 4, 4), device)
    check_tensor("Ks", Ks, torch.float32, (C, 3, 3), device)
    return viewmats, Ks


def tsdf_integrate_raw(vol: "TSDFVolume", frames: Tensor, viewmats: Tensor, Ks: Tensor, alphas: Optional[Tensor] = None,
                       alpha_min: float = 0.5, near: float = 0.01) -> None:
    """mgs_tsdf_integrate on torch's current stream: no synchronisation, no copy.  frames float32 [C,H,W,4] (RGB+ED) or
    [C,H,W] (depth), alphas float32 [C,H,W,1] or [C,H,W] or None, viewmats float32 [C,4,4], Ks float32 [C,3,3], all contiguous
    on the volume's device."""
    dev = vol.tsdf.device
    require_device(frames, alphas, viewmats, Ks)
    if not isinstance(frames, Tensor) or frames.dim() not in (3, 4):
        raise ValueError("frames must be a float32 tensor [C,H,W,4] (an RGB+ED frame) or [C,H,W] (depth)")
    channels = 4 if frames.dim() == 4 else 1
    C, H, W = frames.shape[:3]
    check_tensor("frames", frames, torch.float32, (C, H, W, 4) if channels == 4 else (C, H, W), dev)
    if alphas is not None:
        check_tensor("alphas", alphas, torch.float32, (C, H, W, 1) if alphas.dim() == 4 else (C, H, W), dev)
    check_tensor("viewmats", viewmats, torch.float32, (C, 4, 4), dev)
    check_tensor("Ks", Ks, torch.float32, (C, 3, 3), dev)
    if channels == 1 and vol.color is not None:
        raise ValueError("a depth-only frame carries no colour: fuse it into a volume made with color=False")
    check(_lib.lib().mgs_tsdf_integrate(ctypes.byref(vol._struct()), C, H, W, ptr(frames), channels, ptr(alphas),
                                        float(alpha_min), float(near), ptr(viewmats), ptr(Ks), 0, stream_handle()),
          "mgs_tsdf_integrate")


def tsdf_extract_raw(vol: "TSDFVolume", level: float, min_weight: float, vertex_capacity: Optional[int] = None,
                     face_capacity: Optional[int] = None, guard_rows: int = 0):
    """mgs_tsdf_extract_count, then mgs_tsdf_extract_emit into buffers of the capacities given (None: the counts, read back
    once).  Returns (vertices [cap_v,3], faces [cap_f,3] int32, colors [cap_v,3] | None, counts int64 [2] on the host, status
    uint32 word on the device); with guard_rows each buffer has that many further rows behind its capacity, filled with a
    pattern no output takes, for a test to see that nothing was written there."""
    L, dev, stream = _lib.lib(), vol.tsdf.device, stream_handle()
    v = vol._struct()
    nbytes = ctypes.c_size_t(0)
    check(L.mgs_tsdf_extract_count(ctypes.byref(v), float(level), float(min_weight), None, None, ctypes.byref(nbytes), stream),
          "mgs_tsdf_extract_count(size query)")
    workspace = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=dev)
    pad = -workspace.data_ptr() % 256
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    check(L.mgs_tsdf_extract_count(ctypes.byref(v), float(level), float(min_weight), ptr(counts), workspace.data_ptr() + pad,
                                   ctypes.byref(nbytes), stream), "mgs_tsdf_extract_count")
    n_v, n_f = (int(x) for x in counts.tolist())             # the one read-back: the outputs are sized by it
    cap_v = n_v if vertex_capacity is None else int(vertex_capacity)
    cap_f = n_f if face_capacity is None else int(face_capacity)
    if max(cap_v, cap_f) > 2 ** 31 - 1:
        raise MgsError(f"the surface has {n_v} vertices and {n_f} faces: more than int32 indices address")
    # at least one row behind every pointer: an empty tensor has none, and the entry point refuses NULL
    rows = lambda cap, fill, dtype: torch.full((max(cap + guard_rows, 1), 3), fill, dtype=dtype, device=dev)
    vertices, faces = rows(cap_v, -7.0, torch.float32), rows(cap_f, -7, torch.int32)
    colors = None if vol.color is None else rows(cap_v, -7.0, torch.float32)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(L.mgs_tsdf_extract_emit(ctypes.byref(v), float(level), float(min_weight), ptr(counts), workspace.data_ptr() + pad,
                                  nbytes.value, ptr(vertices), ptr(colors), cap_v, ptr(faces), cap_f, ptr(status), stream),
          "mgs_tsdf_extract_emit")
    return (vertices[:cap_v + guard_rows], faces[:cap_f + guard_rows], None if colors is None else colors[:cap_v + guard_rows],
            (n_v, n_f), status)


def check_extract_status(status: Tensor) -> None:
    """Reads mgs_tsdf_extract_emit's status word back; an overflow of a capacity raises MgsError."""
    if int(status.item()) & _lib.TSDF_STATUS_OVERFLOW:
        raise MgsError("mgs_tsdf_extract_emit: the surface has more vertices or faces than the capacities given "
                       "(MGS_TSDF_STATUS_OVERFLOW); nothing was written past them")


class TSDFVolume:
    """A dense TSDF volume on the GPU: tsdf and weight float32 [nz,ny,nx], color float32 [3,nz,ny,nx] (planar) or None.

    origin: the world position of the volume's low corner; dims = (nx, ny, nz); trunc: the truncation distance (None: three
    voxels); max_weight: the cap of the per-sample observation count, which bounds how slowly old observations fade."""

    def __init__(self, origin: Sequence[float], voxel_size: float, dims: Sequence[int], trunc: Optional[float] = None,
                 color: bool = True, max_weight: float = 64.0, device="cuda"):
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError(f"dims must be three positive integers (nx, ny, nz), got {dims}")
        if dims[0] * dims[1] * dims[2] > 2 ** 31 - 1:
            raise ValueError(f"dims {dims} are more than 2^31 - 1 samples")
        if not float(voxel_size) > 0:
            raise ValueError(f"voxel_size must be positive, got {voxel_size}")
        trunc = 3.0 * float(voxel_size) if trunc is None else float(trunc)
        if not trunc > 0:
            raise ValueError(f"trunc must be positive, got {trunc}")
        if not float(max_weight) >= 1:
            raise ValueError(f"max_weight must be >= 1, got {max_weight}")
        origin = tuple(float(x) for x in origin)
        if len(origin) != 3:
            raise ValueError("origin must be three numbers")
        self.origin, self.voxel_size, self.dims, self.trunc, self.max_weight = origin, float(voxel_size), dims, trunc, float(max_weight)
        device = torch.device(device)
        if device.type != "cuda":
            raise MgsError("a TSDFVolume lives on the GPU: there is no CPU fallback")
        nx, ny, nz = dims
        self.tsdf = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=device) if color else None

    @classmethod
    def from_bounds(cls, lo: Sequence[float], hi: Sequence[float], voxel_size: float, **kwargs) -> "TSDFVolume":
        """The smallest volume of voxel_size that covers the box lo .. hi."""
        if not float(voxel_size) > 0:
            raise ValueError(f"voxel_size must be positive, got {voxel_size}")
        lo, hi = [float(x) for x in lo], [float(x) for x in hi]
        if len(lo) != 3 or len(hi) != 3 or any(h <= l for l, h in zip(lo, hi)):
            raise ValueError(f"bounds must be two corners with lo < hi, got {lo} and {hi}")
        dims = [max(1, math.ceil((h - l) / float(voxel_size) - 1e-6)) for l, h in zip(lo, hi)]
        return cls(lo, voxel_size, dims, **kwargs)

    def _struct(self) -> _lib.TsdfVolume:
        nz, ny, nx = self.tsdf.shape
        dev = self.tsdf.device
        check_tensor("tsdf", self.tsdf, torch.float32, (nz, ny, nx), dev)
        check_tensor("weight", self.weight, torch.float32, (nz, ny, nx), dev)
        if self.color is not None:
            check_tensor("color", self.color, torch.float32, (3, nz, ny, nx), dev)
        return _volume_struct((nx, ny, nz), self.origin, self.voxel_size, self.trunc, self.max_weight, self.tsdf, self.weight,
                              self.color)

    def reset(self) -> "TSDFVolume":
        """Back to the empty volume: every array zero."""
        for t in (self.tsdf, self.weight, self.color):
            if t is not None:
                t.zero_()
        return self

    def integrate(self, frames: Tensor, viewmats, Ks, alphas: Optional[Tensor] = None, alpha_min: float = 0.5,
                  near: float = 0.01, camera_model: str = "pinhole", distortion=None, pinhole_distortion=None) -> "TSDFVolume":
        """Fuse C frames, one launch.  frames: rasterization(render_mode="RGB+ED")'s float32 [C,H,W,4] with its alphas
        [C,H,W,1], both read in place; or a float32 [C,H,W] z-depth tensor alone (sensor depth; the volume must have been
        made with color=False).  viewmats [C,4,4] world-to-camera and Ks [C,3,3]: pinhole cameras, pixel centres at +0.5.
        A pixel is not fused where its depth is not finite or <= 0, or where its alpha is below alpha_min; what such a
        pixel holds, NaN included, changes nothing.  Lens and orthographic cameras: NotImplementedError."""
        if camera_model != "pinhole" or distortion is not None or pinhole_distortion is not None:
            raise NotImplementedError("TSDFVolume.integrate fuses plain pinhole frames only: render the views without "
                                      "camera_model= / distortion= / pinhole_distortion=")
        if not isinstance(frames, Tensor) or frames.dim() not in (3, 4):
            raise ValueError("frames must be a float32 tensor [C,H,W,4] (an RGB+ED frame) or [C,H,W] (depth)")
        viewmats, Ks = _cameras(viewmats, Ks, frames.shape[0], self.tsdf.device)
        tsdf_integrate_raw(self, frames.detach(), viewmats, Ks, None if alphas is None else alphas.detach(), alpha_min, near)
        return self

    def extract_arrays(self, level: float = 0.0, min_weight: float = 1.0) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
        """(vertices float32 [V,3], faces int32 [F,3], colors float32 [V,3] | None) of the isosurface tsdf = level over the cells
        whose eight samples were observed at least min_weight times, possibly with zero rows.  Marching tetrahedra: closed
        where the volume is fully observed, no unreferenced vertex, normals towards free space, and the same arrays for the
        same volume.  An offline step: the two counts are read back once to size the outputs (one synchronisation)."""
        vertices, faces, colors, _, _ = tsdf_extract_raw(self, level, min_weight)
        return vertices, faces, colors

    def extract_mesh(self, level: float = 0.0, min_weight: float = 1.0) -> Mesh:
        """extract_arrays as a Mesh with vertex_colors (where the volume has colour).  ValueError for an empty surface."""
        vertices, faces, colors = self.extract_arrays(level, min_weight)
        if faces.shape[0] == 0:
            raise ValueError(f"the surface is empty: no cell observed {min_weight:g} times or more crosses tsdf = {level:g} "
                             "(nothing fused yet, or the volume does not contain the scene's surfaces)")
        return Mesh(vertices, faces, vertex_colors=colors)


__all__ = ["TSDFVolume", "tsdf_integrate_raw", "tsdf_extract_raw", "check_extract_status"]
