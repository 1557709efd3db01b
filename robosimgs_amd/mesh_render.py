"""Triangle meshes rendered on the GPU (include/mgs_mesh.h, csrc/mesh.hip, csrc/mesh_kernels.h): the opaque foreground of a hybrid frame, as an
operator of its own that the caller composites over a Gaussian render.

    box = Mesh.merge([Mesh.from_glb("lid.glb"), Mesh.from_glb("body.glb")], link_ids=[0, -1]).to("cuda")
    rgb, depth, meta = rasterize_mesh(box, viewmats, Ks, 1280, 720, rotations=R[None], translations=t[None])
    out_rgb, out_depth = composite_over(bg_rgb, bg_alpha, bg_depth, rgb[0], depth[0])

    r = MeshRenderer(box, 1280, 720, headlight=True)           # workspace and outputs allocated once
    rgb, depth, meta = r.render(viewmats, Ks, rotations=R_dev, translations=t_dev)       # launches only

Four stages on torch's current stream, over C cameras: a kernel clears the visibility buffer; the vertex stage poses and
views the vertices (x' = s R x + t for a vertex whose link id is in 0 .. L-1 with L = len(rotations); every other vertex is
static -- a link id >= L is not an error, because finding one would take a read-back); the face stage rasterises with a
64-bit atomic minimum on (depth bits, face index); the resolve stage writes rgb, depth, face ids and optionally normals.
Semantics and fp32 evaluation order: tests/mesh_ref.py.  Nothing synchronises, allocates (in MeshRenderer.render), reads back
or copies from the host; no floating-point atomic: the same inputs give the same bytes in every run.  `depth` is 0 where no
face covers the pixel, which is what composite_over(fg_depth=) takes as absent.

A mesh with textures (Mesh.face_uvs, face_textures, textures) takes the textured resolve (include/mgs_mesh_texture.h,
csrc/mesh_texture.hip; semantics: tests/texture_ref.py): MeshRenderer packs the textures and builds their mipmaps on the GPU
once (build_texture_set), render() keeps its signature, texture_filter= chooses "trilinear" or "bilinear".  A mesh without
textures goes down the untextured entry points, which are unchanged.

Under a lens (camera_model="fisheye", distortion=, pinhole_distortion=: rasterization's keywords) the same triangles are
rasterised at each pixel's own ray, solved from the lens per pixel (include/mgs_mesh_lens.h, csrc/mesh_lens.hip; semantics:
tests/mesh_lens_ref.py): nothing is tessellated or resampled, and the mesh layer registers with a splat frame rendered
under that lens.  mesh_lens_rays builds the ray map as a stage of its own; mesh_raster and mesh_resolve take it as rays=.
The raster and resolve kernels are the pinhole path's own text (csrc/mesh_kernels.h), instantiated for the ray map.

Argument errors are ValueErrors raised before any launch.  There is no fallback: a missing library is an error.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import (MESH_FILTER, MESH_MAX_SIDE, MESH_MAX_TEXTURES, MESH_TEXTURE_DESC_WORDS, MESH_TEXTURE_MAX_SIDE, MESH_WRAP,
                   aligned_workspace, check, ptr, stream_handle)
from .mesh import Mesh, Texture
from .ops import CAMERA_FISHEYE_KB, CAMERA_MODELS, CAMERA_PINHOLE_BC, LENS_ROW_FLOATS, camera_model_id, lens_rows


def _check_sizes(n_cams: int, V: int, F: int, width: int, height: int) -> None:
    if n_cams < 1:
        raise ValueError(f"n_cams {n_cams}: at least one camera is needed")
    if V < 1 or F < 1:
        raise ValueError(f"a mesh of {V} vertices and {F} faces cannot be rasterised: at least one of each is needed")
    if not (1 <= width <= MESH_MAX_SIDE and 1 <= height <= MESH_MAX_SIDE):
        raise ValueError(f"image {width} x {height}: each side must be in 1 .. {MESH_MAX_SIDE}")


def _check_planes(near_plane: float, far_plane: float) -> None:
    if not (near_plane > 0):
        raise ValueError(f"near_plane {near_plane} is not a positive number")
    if not (far_plane >= near_plane):
        raise ValueError(f"far_plane {far_plane} is not a number at or above near_plane {near_plane}")


def _check_ambient(ambient: float) -> None:
    if not (0.0 <= ambient <= 1.0):
        raise ValueError(f"ambient {ambient} is outside 0 .. 1")


def _dev(t, shape: Tuple, dtype, what: str, device=None, nullable: bool = False) -> Optional[Tensor]:
    """A launch-ready tensor or a ValueError: a contiguous `dtype` CUDA tensor of `shape` (-1: any) on `device`."""
    if t is None:
        if nullable:
            return None
        raise ValueError(f"{what} is missing")
    if not torch.is_tensor(t):
        raise ValueError(f"{what} must be a tensor, got {type(t).__name__}")
    if t.dim() != len(shape) or any(s != -1 and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{what} must be {list(shape)} (-1: any), got {list(t.shape)}")
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{what} is a CPU tensor: the mesh rasteriser runs on the GPU only")
    if device is not None and t.device != device:
        raise ValueError(f"{what} is on {t.device}, the mesh is on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t


def _links(rotations, translations, scales, device):
    """(L, rotations [L,3,3], translations [L,3], scales [L] | None), launch-ready."""
    if rotations is None and translations is None:
        if scales is not None:
            raise ValueError("scales given without rotations and translations")
        return 0, None, None, None
    if rotations is None or translations is None:
        raise ValueError("rotations and translations go together: one of them is missing")
    rotations = _dev(rotations, (-1, 3, 3), torch.float32, "rotations", device)
    L = int(rotations.shape[0])
    translations = _dev(translations, (L, 3), torch.float32, "translations", device)
    scales = _dev(scales, (L,), torch.float32, "scales", device, nullable=True)
    return L, rotations, translations, scales


def _workspace(workspace: Optional[Tensor], need: int, device) -> Tuple[Tensor, int]:
    """(the uint8 tensor, the offset of its first 256-byte aligned byte); allocated where none is given."""
    if workspace is not None:
        _dev(workspace, (-1,), torch.uint8, "workspace", device)
    workspace, pad = aligned_workspace(workspace, need, device)
    if workspace.numel() - pad < need:
        raise ValueError(f"workspace of {workspace.numel()} bytes, {need + 256} needed (mesh_workspace_bytes + 256)")
    return workspace, pad


def mesh_workspace_bytes(n_cams: int, n_vertices: int, n_faces: int, width: int, height: int) -> int:
    """mgs_mesh_workspace_bytes: visibility uint64 [C,H,W], a counter per camera, 64 bytes per (camera, face)."""
    _check_sizes(n_cams, n_vertices, n_faces, width, height)
    n = ctypes.c_size_t(0)
    check(_lib.lib().mgs_mesh_workspace_bytes(int(n_cams), int(n_vertices), int(n_faces), int(width), int(height), ctypes.byref(n)),
          "mgs_mesh_workspace_bytes")
    return int(n.value)


def _visibility(workspace: Tensor, pad: int, n_cams: int, width: int, height: int) -> Tensor:
    return workspace[pad:pad + 8 * n_cams * height * width].view(torch.int64).view(n_cams, height, width)


# ---- the lens (include/mgs_mesh_lens.h) ---------------------------------------------------------------------------------------
def _lens_model(camera_model: str, distortion, pinhole_distortion) -> Optional[int]:
    """MGS_CAMERA_FISHEYE_KB or MGS_CAMERA_PINHOLE_BC of rasterization's three camera keywords (their checks are
    ops.camera_model_id's), None for the plain pinhole -- all-zero pinhole_distortion included, as there.  The ideal fisheye is
    MGS_CAMERA_FISHEYE_KB with every k zero.  The orthographic camera has parallel rays and no ray map: NotImplementedError."""
    model = camera_model_id(camera_model, distortion, pinhole_distortion)
    if model == CAMERA_MODELS["ortho"]:
        raise NotImplementedError("camera_model='ortho': the mesh rasteriser has no orthographic camera (its rays are parallel: "
                                  "there is no ray map of the lens path's form)")
    if model == CAMERA_MODELS["pinhole"]:
        return None
    return CAMERA_PINHOLE_BC if model == CAMERA_PINHOLE_BC else CAMERA_FISHEYE_KB


_IDEAL_FISHEYE_TAILS: dict = {}                # device -> [1,7] zeros | theta_max^2 | 0 0: uploaded once per device


def _lens_rows(Ks: Tensor, model: int, distortion, pinhole_distortion) -> Tensor:
    """The [C,16] camera rows of `model` for Ks [C,3,3] on the device (ops.lens_rows; the ideal fisheye's are built here)."""
    if model == CAMERA_PINHOLE_BC:
        return lens_rows(Ks, None, pinhole_distortion)
    if camera_model_id("fisheye", distortion) == CAMERA_FISHEYE_KB:
        return lens_rows(Ks, distortion)
    tail = _IDEAL_FISHEYE_TAILS.get(Ks.device)
    if tail is None:
        from .camera import lens_theta_max
        host = torch.zeros((1, LENS_ROW_FLOATS - 9), dtype=torch.float32)
        host[0, 4] = lens_theta_max([0.0, 0.0, 0.0, 0.0]) ** 2
        tail = _IDEAL_FISHEYE_TAILS[Ks.device] = host.to(Ks.device)
    C = Ks.shape[0]
    return torch.cat([Ks.reshape(C, 9), tail.expand(C, -1)], dim=1).contiguous()


def mesh_lens_workspace_bytes(n_cams: int, width: int, height: int) -> int:
    """mgs_mesh_lens_workspace_bytes: rays float [C,H,W,2], a rectangle per 8 x 8 block and one per 8 x 8 blocks."""
    _check_sizes(n_cams, 1, 1, width, height)
    n = ctypes.c_size_t(0)
    check(_lib.lib().mgs_mesh_lens_workspace_bytes(int(n_cams), int(width), int(height), ctypes.byref(n)),
          "mgs_mesh_lens_workspace_bytes")
    return int(n.value)


class MeshLensMap:
    """The ray map of C cameras under a lens, as mgs_mesh_lens_rays left it in its workspace: model (MGS_CAMERA_*), rows
    float32 [C,16] (the camera rows it was built from), rays float32 [C,H,W,2] (a view of the workspace: (x_u, y_u) per
    pixel, NaN where the pixel has no ray).  mesh_raster(rays=) and mesh_resolve(rays=) take it."""

    def __init__(self, model: int, rows: Tensor, workspace: Tensor, pad: int, n_cams: int, width: int, height: int):
        self.model, self.rows, self.workspace, self.pad = model, rows, workspace, pad
        self.n_cams, self.width, self.height = n_cams, width, height

    @property
    def rays(self) -> Tensor:
        C, H, W = self.n_cams, self.height, self.width
        return self.workspace[self.pad:self.pad + 8 * C * H * W].view(torch.float32).view(C, H, W, 2)

    def _args(self, C: int, width: int, height: int, device):
        if not (self.n_cams == C and self.width == width and self.height == height):
            raise ValueError(f"rays= was built for {self.n_cams} cameras at {self.width} x {self.height}, the call is for {C} at "
                             f"{width} x {height}")
        if self.workspace.device != device:
            raise ValueError(f"rays= is on {self.workspace.device}, the mesh is on {device}")
        return self.model, ptr(self.rows), self.workspace.data_ptr() + self.pad, self.workspace.numel() - self.pad


def _lens_map(rays, C: int, width: int, height: int, device):
    if not isinstance(rays, MeshLensMap):
        raise ValueError(f"rays must be a MeshLensMap (mesh_lens_rays), got {type(rays).__name__}")
    return rays._args(C, width, height, device)


@torch.no_grad()
def mesh_lens_rays(Ks: Tensor, width: int, height: int, camera_model: str = "pinhole", distortion=None, pinhole_distortion=None,
                   workspace: Optional[Tensor] = None) -> MeshLensMap:
    """mgs_mesh_lens_rays: the per-pixel rays of C cameras under a lens and their block tables, as a MeshLensMap.  Ks float32
    [C,3,3] on the GPU; camera_model, distortion (fisheye k1..k4) and pinhole_distortion (k1 k2 p1 p2 k3) as rasterization
    takes them.  workspace: a uint8 tensor of mesh_lens_workspace_bytes(...) + 256 bytes, allocated where None.  A camera
    without a lens (the plain pinhole) has no ray map: ValueError."""
    model = _lens_model(camera_model, distortion, pinhole_distortion)
    if model is None:
        raise ValueError("mesh_lens_rays needs a lens: the plain pinhole camera goes down mesh_raster / mesh_resolve with Ks")
    Ks = _dev(Ks, (-1, 3, 3), torch.float32, "Ks")
    C, width, height = int(Ks.shape[0]), int(width), int(height)
    _check_sizes(C, 1, 1, width, height)
    rows = _lens_rows(Ks, model, distortion, pinhole_distortion)
    workspace, pad = _workspace(workspace, mesh_lens_workspace_bytes(C, width, height), Ks.device)
    check(_lib.lib().mgs_mesh_lens_rays(C, model, ptr(rows), width, height, workspace.data_ptr() + pad, workspace.numel() - pad,
                                        stream_handle()), "mgs_mesh_lens_rays")
    return MeshLensMap(model, rows, workspace, pad, C, width, height)


# ---- textures (include/mgs_mesh_texture.h) -----------------------------------------------------------------------------------
def _filter(texture_filter: str) -> int:
    if texture_filter not in MESH_FILTER:
        raise ValueError(f"texture_filter must be 'trilinear' or 'bilinear', got {texture_filter!r}")
    return MESH_FILTER[texture_filter]


class TextureSet:
    """The textures of a mesh on the device, built once: descriptors int32 [T,20] (host copy: descriptors_host) and texels
    int32 [texel_count], one word per texel, every level of every texture (include/mgs_mesh_texture.h has the layout).
    level(t, l) is a uint8 view [h_l, w_l, 4] of one level."""

    def __init__(self, descriptors_host: Tensor, descriptors: Tensor, texels: Tensor, mipmaps: bool):
        self.descriptors_host, self.descriptors, self.texels, self.mipmaps = descriptors_host, descriptors, texels, mipmaps
        self.n_textures, self.texel_count, self.device = int(descriptors.shape[0]), int(texels.numel()), texels.device

    def level(self, t: int, l: int) -> Tensor:
        w, h, levels = (int(v) for v in self.descriptors_host[t, :3])
        if not 0 <= l < levels:
            raise ValueError(f"texture {t} has {levels} levels, level {l} was asked for")
        at, wl, hl = int(self.descriptors_host[t, 4 + l]) & 0xFFFFFFFF, max(1, w >> l), max(1, h >> l)
        return self.texels[at:at + wl * hl].view(torch.uint8).view(hl, wl, 4)


@torch.no_grad()
def build_texture_set(textures, device, mipmaps: bool = True) -> TextureSet:
    """Pack `textures` (a list of Texture) for the textured resolve: the descriptors and level 0 of every texture are copied to
    `device` here, once; with mipmaps the other levels are built there (mgs_mesh_build_mips, one launch per level and texture),
    without them every texture is described as its level 0 alone, so trilinear filtering degrades to bilinear."""
    textures = list(textures)
    if not textures or not all(isinstance(t, Texture) for t in textures):
        raise ValueError("textures must be a non-empty list of Texture")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"a texture set lives on the GPU, got device {device}")
    T = len(textures)
    if T > MESH_MAX_TEXTURES:
        raise ValueError(f"{T} textures, at most {MESH_MAX_TEXTURES} in a set")
    for k, t in enumerate(textures):
        if not (1 <= t.width <= MESH_TEXTURE_MAX_SIDE and 1 <= t.height <= MESH_TEXTURE_MAX_SIDE):
            raise ValueError(f"texture {k} is {t.width} x {t.height}: each side must be in 1 .. {MESH_TEXTURE_MAX_SIDE}")
    sizes = torch.tensor([[t.width, t.height] for t in textures], dtype=torch.int32)
    wraps = torch.tensor([[MESH_WRAP[t.wrap_s], MESH_WRAP[t.wrap_t]] for t in textures], dtype=torch.int32)
    desc = torch.zeros((T, MESH_TEXTURE_DESC_WORDS), dtype=torch.int32)
    n = ctypes.c_size_t(0)
    L = _lib.lib()
    check(L.mgs_mesh_texture_layout(T, sizes.data_ptr(), wraps.data_ptr(), desc.data_ptr(), ctypes.byref(n)), "mgs_mesh_texture_layout")
    if not mipmaps:
        # level 0 of every texture alone, packed: the same call on 1 x 1 "levels" does not exist, so lay them out here
        at = 0
        for k, t in enumerate(textures):
            desc[k, 2], desc[k, 4], desc[k, 5:] = 1, at, 0
            at += t.width * t.height
        if at >= 2 ** 31:
            raise ValueError(f"the textures hold {at} texels, fewer than 2^31 are allowed")
        n = ctypes.c_size_t(at)
    texels = torch.empty(int(n.value), dtype=torch.int32, device=device)
    for k, t in enumerate(textures):
        at = int(desc[k, 4]) & 0xFFFFFFFF
        texels[at:at + t.width * t.height].view(torch.uint8).view(t.height, t.width, 4).copy_(t.image)
    if mipmaps:
        check(L.mgs_mesh_build_mips(T, desc.data_ptr(), ptr(texels), int(n.value), stream_handle()), "mgs_mesh_build_mips")
    return TextureSet(desc, desc.to(device), texels, bool(mipmaps))


def _texture_args(textures, face_uvs, face_textures, F: int, dev):
    """The seven trailing arguments of the textured entry points before filter and stream, launch-ready."""
    if not isinstance(textures, TextureSet):
        raise ValueError(f"textures must be a TextureSet (build_texture_set), got {type(textures).__name__}")
    if textures.device != dev:
        raise ValueError(f"the texture set is on {textures.device}, the mesh is on {dev}")
    face_uvs = _dev(face_uvs, (F, 3, 2), torch.float32, "face_uvs", dev)
    face_textures = _dev(face_textures, (F,), torch.int32, "face_textures", dev)
    return (ptr(face_uvs), ptr(face_textures), textures.n_textures, ptr(textures.descriptors), ptr(textures.texels),
            textures.texel_count)


# ---- stage operators (each mirrors one entry point; no synchronisation) ---------------------------------------------------
@torch.no_grad()
def mesh_vertices(vertices: Tensor, viewmats: Tensor, link_ids: Optional[Tensor] = None, rotations: Optional[Tensor] = None,
                  translations: Optional[Tensor] = None, scales: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """mgs_mesh_vertices: verts_cam float32 [C,V,3].  vertices float32 [V,3], viewmats float32 [C,4,4], link_ids int32 [V] or
    None (all static), rotations float32 [L,3,3], translations [L,3], scales [L] or None; a link id outside 0 .. L-1 is static."""
    vertices = _dev(vertices, (-1, 3), torch.float32, "vertices")
    dev, V = vertices.device, int(vertices.shape[0])
    viewmats = _dev(viewmats, (-1, 4, 4), torch.float32, "viewmats", dev)
    C = int(viewmats.shape[0])
    _check_sizes(C, V, 1, 1, 1)
    link_ids = _dev(link_ids, (V,), torch.int32, "link_ids", dev, nullable=True)
    L, rotations, translations, scales = _links(rotations, translations, scales, dev)
    if out is None:
        out = torch.empty((C, V, 3), dtype=torch.float32, device=dev)
    else:
        _dev(out, (C, V, 3), torch.float32, "out", dev)
    check(_lib.lib().mgs_mesh_vertices(C, V, ptr(vertices), ptr(link_ids), L, ptr(rotations), ptr(translations), ptr(scales),
                                       ptr(viewmats), ptr(out), stream_handle()), "mgs_mesh_vertices")
    return out


@torch.no_grad()
def mesh_raster(verts_cam: Tensor, faces: Tensor, Ks: Tensor, width: int, height: int, near_plane: float = 0.01,
                far_plane: float = 1e10, cull_backfaces: bool = False, workspace: Optional[Tensor] = None,
                rays: Optional[MeshLensMap] = None) -> Tuple[Tensor, Tensor]:
    """mgs_mesh_raster (clear + faces): (visibility, workspace).  visibility is an int64 view [C,H,W] of the workspace's first
    field: the bits of (float_bits(z) << 32) | face per pixel, -1 (all ones) where uncovered.  workspace: a uint8 tensor of
    mesh_workspace_bytes(...) + 256 bytes, allocated where None; hand it to mesh_resolve.  rays (mesh_lens_rays): rasterise
    under that lens (mgs_mesh_raster_lens); the map carries the camera, Ks is then only checked."""
    verts_cam = _dev(verts_cam, (-1, -1, 3), torch.float32, "verts_cam")
    dev, C, V = verts_cam.device, int(verts_cam.shape[0]), int(verts_cam.shape[1])
    faces = _dev(faces, (-1, 3), torch.int32, "faces", dev)
    F, width, height = int(faces.shape[0]), int(width), int(height)
    _check_sizes(C, V, F, width, height)
    _check_planes(near_plane, far_plane)
    Ks = _dev(Ks, (C, 3, 3), torch.float32, "Ks", dev)
    lens = None if rays is None else _lens_map(rays, C, width, height, dev)
    need = mesh_workspace_bytes(C, V, F, width, height)
    workspace, pad = _workspace(workspace, need, dev)
    if rays is None:
        check(_lib.lib().mgs_mesh_raster(C, V, ptr(verts_cam), F, ptr(faces), ptr(Ks), width, height, float(near_plane),
                                         float(far_plane), int(bool(cull_backfaces)), workspace.data_ptr() + pad,
                                         workspace.numel() - pad, stream_handle()), "mgs_mesh_raster")
    else:
        model, rows, lens_ws, lens_bytes = lens
        check(_lib.lib().mgs_mesh_raster_lens(C, V, ptr(verts_cam), F, ptr(faces), model, rows, width, height, float(near_plane),
                                              float(far_plane), int(bool(cull_backfaces)), workspace.data_ptr() + pad,
                                              workspace.numel() - pad, lens_ws, lens_bytes, stream_handle()),
              "mgs_mesh_raster_lens")
    return _visibility(workspace, pad, C, width, height), workspace


def _outputs(out: Optional[Dict], C: int, height: int, width: int, normals: bool, dev) -> Dict:
    res = dict(out) if out is not None else {}
    want = {"rgb": ((C, height, width, 3), torch.float32), "depth": ((C, height, width), torch.float32),
            "face_ids": ((C, height, width), torch.int32)}
    if normals:
        want["normals"] = ((C, height, width, 3), torch.float32)
    for name, (shape, dtype) in want.items():
        if res.get(name) is None:
            res[name] = torch.empty(shape, dtype=dtype, device=dev)
        else:
            _dev(res[name], shape, dtype, f"out[{name!r}]", dev)
    return res


@torch.no_grad()
def mesh_resolve(verts_cam: Tensor, faces: Tensor, Ks: Tensor, width: int, height: int, workspace: Tensor,
                 vertex_colors: Optional[Tensor] = None, face_colors: Optional[Tensor] = None, headlight: bool = False,
                 ambient: float = 0.3, return_normals: bool = False, out: Optional[Dict] = None, *,
                 textures: Optional[TextureSet] = None, face_uvs: Optional[Tensor] = None,
                 face_textures: Optional[Tensor] = None, texture_filter: str = "trilinear",
                 rays: Optional[MeshLensMap] = None) -> Dict:
    """mgs_mesh_resolve on the workspace mesh_raster left: dict(rgb float32 [C,H,W,3], depth float32 [C,H,W], face_ids int32
    [C,H,W] and, with return_normals, normals float32 [C,H,W,3]).  Uncovered pixels are (0, 0, 0), 0 and -1.

    textures (a TextureSet) with face_uvs float32 [F,3,2] and face_textures int32 [F] goes through mgs_mesh_resolve_textured:
    rgb = texel x tint x shade where the face is textured (texture_filter "trilinear" or "bilinear"), the same bits as
    without textures everywhere else.  Without textures this is the untextured entry point, unchanged.

    rays (mesh_lens_rays, the map mesh_raster was given): mgs_mesh_resolve_lens; a pixel without a ray is uncovered.  Textures
    under a lens are not built (their level of detail needs the ray map's derivatives): NotImplementedError."""
    verts_cam = _dev(verts_cam, (-1, -1, 3), torch.float32, "verts_cam")
    dev, C, V = verts_cam.device, int(verts_cam.shape[0]), int(verts_cam.shape[1])
    faces = _dev(faces, (-1, 3), torch.int32, "faces", dev)
    F, width, height = int(faces.shape[0]), int(width), int(height)
    _check_sizes(C, V, F, width, height)
    _check_ambient(ambient)
    Ks = _dev(Ks, (C, 3, 3), torch.float32, "Ks", dev)
    vertex_colors = _dev(vertex_colors, (V, 3), torch.float32, "vertex_colors", dev, nullable=True)
    face_colors = _dev(face_colors, (F, 3), torch.float32, "face_colors", dev, nullable=True)
    workspace, pad = _workspace(_dev(workspace, (-1,), torch.uint8, "workspace", dev), mesh_workspace_bytes(C, V, F, width, height), dev)
    res = _outputs(out, C, height, width, return_normals, dev)
    args = (C, V, ptr(verts_cam), F, ptr(faces), ptr(vertex_colors), ptr(face_colors), ptr(Ks), width, height,
            int(bool(headlight)), float(ambient), workspace.data_ptr() + pad, workspace.numel() - pad, ptr(res["rgb"]),
            ptr(res["depth"]), ptr(res["face_ids"]), ptr(res.get("normals")))
    if rays is not None:
        if textures is not None:
            raise NotImplementedError("a textured mesh under a lens is not built: the texture's level of detail needs the ray "
                                      "map's derivatives")
        model, rows, lens_ws, lens_bytes = _lens_map(rays, C, width, height, dev)
        check(_lib.lib().mgs_mesh_resolve_lens(*args[:7], model, rows, *args[8:14], lens_ws, lens_bytes, *args[14:],
                                               stream_handle()), "mgs_mesh_resolve_lens")
    elif textures is None:
        if face_uvs is not None or face_textures is not None:
            raise ValueError("face_uvs and face_textures need textures=")
        check(_lib.lib().mgs_mesh_resolve(*args, stream_handle()), "mgs_mesh_resolve")
    else:
        filt = _filter(texture_filter)
        tex = _texture_args(textures, face_uvs, face_textures, F, dev)
        check(_lib.lib().mgs_mesh_resolve_textured(*args, *tex, filt, stream_handle()), "mgs_mesh_resolve_textured")
    return res


# ---- the renderer -------------------------------------------------------------------------------------------------------------
class MeshRenderer:
    """A mesh, an image size and a camera count with everything allocated once: the workspace, verts_cam [C,V,3] and the
    outputs.  render() checks its arguments and launches (mgs_rasterize_mesh: five launches on torch's current stream): no
    allocation, no copy, no synchronisation, so it can be captured in a graph of its own and replayed with viewmats, Ks
    and the link transforms overwritten in place.  Every call writes the same output tensors.

    options: near_plane=0.01, far_plane=1e10, cull_backfaces=False, headlight=False, ambient=0.3, return_normals=False;
    out: dict of preallocated outputs (rgb, depth, face_ids, normals), workspace: a uint8 tensor of
    mesh_workspace_bytes(...) + 256 bytes.

    The camera: camera_model="pinhole" | "fisheye", distortion= (fisheye k1..k4) and pinhole_distortion= (OpenCV k1 k2 p1 p2
    k3) with the meaning and the checks of rasterization's keywords, so that a mesh layer registers with a splat frame
    rendered under the same lens.  Without a lens (all-zero pinhole coefficients included) this is the plain pinhole path,
    unchanged.  Under a lens render() goes through mgs_rasterize_mesh_lens (include/mgs_mesh_lens.h; eight launches): every
    pixel's ray is solved from the lens in every call (Ks may be overwritten in place between frames), meta["rays"] is that
    map, float32 [C,H,W,2], NaN where the lens has no ray, and such a pixel is uncovered.  render() then builds the camera
    rows from Ks (one small allocation).  A textured mesh under a lens and camera_model="ortho" raise NotImplementedError."""

    def __init__(self, mesh: Mesh, width: int, height: int, n_cams: int = 1, *, near_plane: float = 0.01,
                 far_plane: float = 1e10, cull_backfaces: bool = False, headlight: bool = False, ambient: float = 0.3,
                 return_normals: bool = False, out: Optional[Dict] = None, workspace: Optional[Tensor] = None,
                 texture_filter: str = "trilinear", camera_model: str = "pinhole", distortion=None, pinhole_distortion=None):
        if not isinstance(mesh, Mesh):
            raise ValueError(f"mesh must be a Mesh, got {type(mesh).__name__}")
        self.lens_model = _lens_model(camera_model, distortion, pinhole_distortion)
        self._distortion, self._pinhole_distortion = distortion, pinhole_distortion
        if self.lens_model is not None and mesh.has_textures:
            raise NotImplementedError("a textured mesh under a lens is not built: the texture's level of detail needs the ray "
                                      "map's derivatives")
        self.width, self.height, self.n_cams = int(width), int(height), int(n_cams)
        _check_sizes(self.n_cams, mesh.n_vertices, mesh.n_faces, self.width, self.height)
        _check_planes(near_plane, far_plane)
        _check_ambient(ambient)
        if mesh.device.type != "cuda":
            raise ValueError(f"the mesh is on {mesh.device} (CPU tensors): the mesh rasteriser runs on the GPU only, use mesh.to('cuda')")
        self.mesh, self.device = mesh, mesh.device
        self.near_plane, self.far_plane, self.ambient = float(near_plane), float(far_plane), float(ambient)
        self.cull_backfaces, self.headlight, self.return_normals = bool(cull_backfaces), bool(headlight), bool(return_normals)
        V, F, C = mesh.n_vertices, mesh.n_faces, self.n_cams
        self._vertices = _dev(mesh.vertices, (V, 3), torch.float32, "mesh.vertices")
        self._faces = _dev(mesh.faces, (F, 3), torch.int32, "mesh.faces", self.device)
        self._vcol = _dev(mesh.vertex_colors, (V, 3), torch.float32, "mesh.vertex_colors", self.device, nullable=True)
        self._fcol = _dev(mesh.face_colors, (F, 3), torch.float32, "mesh.face_colors", self.device, nullable=True)
        self._link = _dev(mesh.link_ids, (V,), torch.int32, "mesh.link_ids", self.device, nullable=True)
        self.workspace_bytes = mesh_workspace_bytes(C, V, F, self.width, self.height)
        self.workspace, self._pad = _workspace(workspace, self.workspace_bytes, self.device)
        self.verts_cam = torch.empty((C, V, 3), dtype=torch.float32, device=self.device)
        self.out = _outputs(out, C, self.height, self.width, self.return_normals, self.device)
        self.lens_workspace = None
        if self.lens_model is not None:
            self.lens_workspace, self._lens_pad = _workspace(None, mesh_lens_workspace_bytes(C, self.width, self.height), self.device)
        # a textured mesh: the texture set is packed and its mips built here, once; render() then takes the textured entry point
        self._filter = _filter(texture_filter)
        self.textures = build_texture_set(mesh.textures, self.device) if mesh.has_textures else None
        self._tex = None if self.textures is None else _texture_args(self.textures, mesh.face_uvs, mesh.face_textures, F, self.device)

    @torch.no_grad()
    def render(self, viewmats: Tensor, Ks: Tensor, rotations: Optional[Tensor] = None, translations: Optional[Tensor] = None,
               scales: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Dict]:
        """viewmats float32 [C,4,4] (world to camera), Ks float32 [C,3,3], rotations float32 [L,3,3], translations [L,3],
        scales [L] or None: contiguous tensors on the mesh's device.  Link l of the mesh takes transform l; a link id >= L
        (or < 0) is static.  Returns (rgb [C,H,W,3], depth [C,H,W], meta) with meta = dict(face_ids int32 [C,H,W], verts_cam
        [C,V,3][, normals [C,H,W,3]]): the renderer's own tensors, overwritten by the next call.  Under a lens also rays
        float32 [C,H,W,2] (NaN where the lens has no ray) and lens_map, the MeshLensMap that mesh_raster(rays=) takes."""
        C, m = self.n_cams, self.mesh
        viewmats = _dev(viewmats, (C, 4, 4), torch.float32, "viewmats", self.device)
        Ks = _dev(Ks, (C, 3, 3), torch.float32, "Ks", self.device)
        L, rotations, translations, scales = _links(rotations, translations, scales, self.device)
        o = self.out
        args = (C, m.n_vertices, ptr(self._vertices), ptr(self._link), L, ptr(rotations), ptr(translations), ptr(scales),
                ptr(viewmats), ptr(Ks), m.n_faces, ptr(self._faces), ptr(self._vcol), ptr(self._fcol), self.width, self.height,
                self.near_plane, self.far_plane, int(self.cull_backfaces), int(self.headlight), self.ambient,
                self.workspace.data_ptr() + self._pad, self.workspace.numel() - self._pad, ptr(self.verts_cam), ptr(o["rgb"]),
                ptr(o["depth"]), ptr(o["face_ids"]), ptr(o.get("normals")))
        meta = {"face_ids": o["face_ids"], "verts_cam": self.verts_cam}
        if self.lens_model is not None:
            rows = _lens_rows(Ks, self.lens_model, self._distortion, self._pinhole_distortion)
            lens = MeshLensMap(self.lens_model, rows, self.lens_workspace, self._lens_pad, C, self.width, self.height)
            check(_lib.lib().mgs_rasterize_mesh_lens(*args[:9], self.lens_model, ptr(rows), *args[10:23],
                                                     self.lens_workspace.data_ptr() + self._lens_pad,
                                                     self.lens_workspace.numel() - self._lens_pad, *args[23:], stream_handle()),
                  "mgs_rasterize_mesh_lens")
            meta["rays"], meta["lens_map"] = lens.rays, lens
        elif self._tex is None:
            check(_lib.lib().mgs_rasterize_mesh(*args, stream_handle()), "mgs_rasterize_mesh")
        else:
            check(_lib.lib().mgs_rasterize_mesh_textured(*args, *self._tex, self._filter, stream_handle()),
                  "mgs_rasterize_mesh_textured")
        if self.return_normals:
            meta["normals"] = o["normals"]
        return o["rgb"], o["depth"], meta

def _to_device(x, dtype, device):
    """A host array, list or tensor of any float dtype as a contiguous `dtype` tensor on `device` (None stays None)."""
    if x is None:
        return None
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    return x.to(device=device, dtype=dtype).contiguous()


def rasterize_mesh(mesh: Mesh, viewmats, Ks, width: int, height: int, *, rotations=None, translations=None, scales=None,
                   near_plane: float = 0.01, far_plane: float = 1e10, cull_backfaces: bool = False, headlight: bool = False,
                   ambient: float = 0.3, return_normals: bool = False, out: Optional[Dict] = None,
                   workspace: Optional[Tensor] = None, texture_filter: str = "trilinear", camera_model: str = "pinhole",
                   distortion=None, pinhole_distortion=None) -> Tuple[Tensor, Tensor, Dict]:
    """Render `mesh` (on the GPU) from C cameras: (rgb float32 [C,H,W,3], depth float32 [C,H,W], meta) with meta =
    dict(face_ids int32 [C,H,W] (-1 where uncovered), verts_cam float32 [C,V,3][, normals float32 [C,H,W,3]]).

    viewmats [C,4,4] (or [4,4]) and Ks [C,3,3] (or [3,3]): tensors or arrays of any float type; an OpenCV pinhole camera,
    or with camera_model= / distortion= / pinhole_distortion= (rasterization's keywords, with its checks) the same lens a
    splat frame was rendered under: every pixel's ray is then solved from the lens, meta["rays"] float32 [C,H,W,2] is that
    map (NaN where the lens has no ray: the pixel is uncovered), and the mesh registers with the frame.  All-zero
    coefficients select the plain path, as there.  A textured mesh under a lens and camera_model="ortho": NotImplementedError.
    rotations [L,3,3], translations [L,3], scales [L]: the convention of transform_gaussians (x' = s R x + t for the
    vertices of link l), so Hinge.pose(angle) feeds them directly (R [3,3] and t [3] are one link).  Link ids >= L are
    static: len(rotations) < mesh.n_links() is not an error, because finding it would take a read-back.
    depth is the z-depth of the nearest face, 0 where there is none: what composite_over(fg_depth=) takes as it stands.
    rgb: vertex colours interpolated, else face colours, else 0.7 grey; headlight=True multiplies by ambient +
    (1 - ambient) |cos| between the face normal and the pixel's ray.  A mesh with textures: rgb = texel x tint x shade on its
    textured faces (tint: the vertex or face colour, else 1), filtered by texture_filter ("trilinear" with mipmaps, or
    "bilinear"); the texture set is packed and its mips built in this call -- MeshRenderer does that once.  out / workspace:
    buffers of an earlier call to reuse (see MeshRenderer, which also keeps the checks and conversions out of a per-frame
    loop)."""
    if not isinstance(mesh, Mesh):
        raise ValueError(f"mesh must be a Mesh, got {type(mesh).__name__}")
    for what, x in (("viewmats", viewmats), ("Ks", Ks)):
        if x is None:
            raise ValueError(f"{what} is missing")
    vm, K = torch.as_tensor(viewmats), torch.as_tensor(Ks)
    vm = vm[None] if vm.dim() == 2 else vm
    K = K[None] if K.dim() == 2 else K
    if vm.dim() != 3 or tuple(vm.shape[1:]) != (4, 4):
        raise ValueError(f"viewmats must be [C,4,4], got {list(vm.shape)}")
    if tuple(K.shape) != (vm.shape[0], 3, 3):
        raise ValueError(f"Ks must be [{vm.shape[0]},3,3], got {list(K.shape)}")
    if not vm.dtype.is_floating_point or not K.dtype.is_floating_point:
        raise ValueError(f"viewmats and Ks must be floating-point, got {vm.dtype} and {K.dtype}")
    if rotations is not None and translations is not None:
        rotations, translations = torch.as_tensor(rotations), torch.as_tensor(translations)
        if rotations.dim() == 2 and translations.dim() == 1:
            rotations, translations = rotations[None], translations[None]
        if rotations.dim() != 3 or tuple(rotations.shape[1:]) != (3, 3) or tuple(translations.shape) != (rotations.shape[0], 3):
            raise ValueError(f"rotations must be [L,3,3] and translations [L,3], got {list(rotations.shape)} and "
                             f"{list(translations.shape)}")
        if scales is not None and tuple(torch.as_tensor(scales).shape) != (rotations.shape[0],):
            raise ValueError(f"scales must be [{rotations.shape[0]}], got {list(torch.as_tensor(scales).shape)}")
    r = MeshRenderer(mesh, width, height, int(vm.shape[0]), near_plane=near_plane, far_plane=far_plane,
                     cull_backfaces=cull_backfaces, headlight=headlight, ambient=ambient, return_normals=return_normals,
                     out=out, workspace=workspace, texture_filter=texture_filter, camera_model=camera_model,
                     distortion=distortion, pinhole_distortion=pinhole_distortion)
    f32 = lambda x: _to_device(x, torch.float32, r.device)
    return r.render(f32(vm), f32(K), rotations=f32(rotations), translations=f32(translations), scales=f32(scales))


__all__ = ["MeshRenderer", "rasterize_mesh", "mesh_vertices", "mesh_raster", "mesh_resolve", "mesh_workspace_bytes",
           "TextureSet", "build_texture_set", "mesh_lens_rays", "mesh_lens_workspace_bytes", "MeshLensMap"]
