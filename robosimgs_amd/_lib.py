"""ctypes binding of libmgs.so (the C ABI declared in include/mgs.h).

There is no fallback: if the shared library is missing or fails to load, importing the ops
raises.  torch is imported first so that libmgs.so binds to the HIP runtime torch already
loaded (same soname, libamdhip64.so.7) and shares its streams and allocations.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p, POINTER

import torch  # noqa: F401  (must precede the dlopen below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmgs.so")
# the same sources built with -DMGS_DEBUG_HOOKS: the only build that has the process-global mgs_debug_set_* knobs
DEBUG_LIB_PATH = os.path.join(_HERE, "csrc", "libmgs_debug.so")
DEBUG_HOOKS = ["mgs_debug_set_raster_cull", "mgs_debug_set_raster_opts", "mgs_debug_set_sort_opts"]

MGS_STATUS_ISECT_OVERFLOW = 1
MGS_SSIM_VALID, MGS_SSIM_SAME = 0, 1       # mgs_image_loss.padding
MGS_VERSION = 450          # include/mgs.h this binding was written against (parameter lists change with it)


class ImageLoss(ctypes.Structure):
    """mgs_image_loss: the image layout and SSIM weight that turn the L1 entry points into L1 + D-SSIM."""
    _fields_ = [("images", c_int), ("height", c_int), ("width", c_int), ("channels", c_int),
                ("ssim_weight", c_float), ("padding", c_int)]


class RgbdLoss(ctypes.Structure):
    """mgs_rgbd_loss (include/mgs_loss_rgbd.h): the frame layout and weights of the masked RGB-D loss."""
    _fields_ = [("images", c_int), ("height", c_int), ("width", c_int), ("render_channels", c_int),
                ("ssim_weight", c_float), ("padding", c_int), ("depth_weight", c_float)]


class AdamGroup(ctypes.Structure):
    """mgs_adam_group (include/mgs_optim.h): one parameter group of mgs_adam_step, n rows of row_floats floats."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("n", c_int64), ("row_floats", c_int32), ("head_floats", c_int32), ("lr", c_double),
                ("lr_final", c_double), ("decay_steps", c_int32), ("rest_lr_scale", c_double)]


ADAM_MAX_GROUPS = 8        # MGS_ADAM_MAX_GROUPS


class RefineGroup(ctypes.Structure):
    """mgs_refine_group (include/mgs_refine.h): one parameter group of mgs_mcmc_relocate, rows of row_floats floats."""
    _fields_ = [("param", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("row_floats", c_int32)]


class McmcStats(ctypes.Structure):
    """mgs_mcmc_stats: what the weights pass leaves on the device (the layout of a 16-byte device buffer)."""
    _fields_ = [("total", c_double), ("n_dead", c_int32), ("n_live", c_int32)]


class TsdfVolume(ctypes.Structure):
    """mgs_tsdf_volume (include/mgs_tsdf.h): the grid, its truncation and weight cap, and its three arrays."""
    _fields_ = [("nx", c_int), ("ny", c_int), ("nz", c_int), ("origin", c_float * 3), ("voxel_size", c_float),
                ("trunc", c_float), ("max_weight", c_float), ("tsdf", c_void_p), ("weight", c_void_p), ("color", c_void_p)]


TSDF_STATUS_OVERFLOW = 1                   # MGS_TSDF_STATUS_OVERFLOW
MCMC_RELOCATE, MCMC_ADD = 0, 1             # mgs_mcmc_relocate.mode
MCMC_MAX_RATIO = 51                        # MGS_MCMC_MAX_RATIO
REFINE_MAX_GROUPS = 8                      # MGS_REFINE_MAX_GROUPS

# every function include/mgs.h declares: name -> (argtypes, restype)
p, i, f, u32 = c_void_p, c_int, c_float, c_uint32
img = POINTER(ImageLoss)
_SIGNATURES = {
    "mgs_version": ([], c_int),
    "mgs_last_error_string": ([], c_char_p),
    "mgs_projection_fwd": ([i, p, p, p, p, p, i, i, f, f, f, f, p, p, p, p, p, p, i, p, i, p], c_int),
    "mgs_projection_bwd": ([i, p, p, p, p, p, i, i, f, p, p, p, p, p, p, p, p, p, p, p, i, p], c_int),
    "mgs_sh_fwd": ([i, i, i, p, p, p, p, p], c_int),
    "mgs_sh_bwd": ([i, i, i, p, p, p, p, p, p, p], c_int),
    "mgs_project_color_fwd": ([i, p, p, p, p, i, i, p, p, p, i, i, f, f, f, f, p, p, p, p, p, i, p, p, i, p, p, p, p], c_int),
    "mgs_project_color_bwd": ([i, p, p, p, p, i, i, p, p, p, i, i, f, p, p, i, i, p, p, p, p, p, p, p, p, p, p, p, p, i, i, p], c_int),
    "mgs_isect_tiles": ([i, p, p, p, p, p, p, i, i, i, i, i, u32, p, p, p, p, p, p, p, p, p, p, p, p, p, POINTER(c_size_t), p], c_int),
    "mgs_isect_offset_encode": ([u32, p, i, i, i, p, p], c_int),
    "mgs_render_frames": ([i, p, p, p, p, i, i, p, i, p, p, i, i, f, f, f, f, i, i, i, p, u32, p, p, p, p, p, p, i, p, p, POINTER(c_size_t), p], c_int),
    "mgs_train_state_layout": ([i, i, i, i, u32, i, i, POINTER(c_size_t), POINTER(c_size_t)], c_int),
    "mgs_render_frames_train": ([i, p, p, p, p, i, i, p, i, p, p, i, i, f, f, f, f, i, i, i, p, u32, i, p, p, p, p, POINTER(c_size_t), p], c_int),
    "mgs_render_frames_backward": ([i, p, p, p, p, i, i, p, i, p, p, i, i, f, i, i, i, p, u32, i, p, p, p, p, p, p, p, p, p, p, p, p, p, p, POINTER(c_size_t), p], c_int),
    "mgs_rasterize_fwd": ([i, p, p, p, p, p, p, i, i, i, i, i, p, p, p, i, p, p, p, p, i, p, p, i, p, p], c_int),
    "mgs_raster_checkpoint_floats": ([u32, i, i, i, i], c_size_t),
    "mgs_rasterize_bwd": ([i, p, p, p, p, p, i, i, i, i, i, p, p, p, p, p, p, p, p, p, p, p, p], c_int),
    "mgs_composite_over": ([i, p, p, p, p, p, p, p, p, p, p], c_int),
    "mgs_points_project": ([i, p, p, p, p, p, p], c_int),
    "mgs_points_depth_map": ([i, p, i, p, i, i, i, i, f, f, p, p, p, POINTER(c_size_t), p], c_int),
    "mgs_points_sample_mask": ([i, p, i, p, i, i, f, p, p, f, p, p], c_int),
    "mgs_frame_to_u8": ([i, p, i, p, p, p, p], c_int),
    "mgs_frame_to_dataset": ([i, i, p, i, p, p, p, p, p, i, p], c_int),
    "mgs_transform_gaussians": ([i, p, p, p, i, i, p, p, i, p, p, p, p, p, p, p], c_int),
    "mgs_l1_loss_fwd": ([c_size_t, p, p, p, p, POINTER(c_size_t), p, img], c_int),
    "mgs_l1_loss_bwd": ([c_size_t, p, p, p, p, p, img], c_int),
    "mgs_l1_loss_fwd_grad": ([c_size_t, p, p, p, p, p, POINTER(c_size_t), p, img], c_int),
    "mgs_l1_loss_bwd_scale": ([c_size_t, p, p, p], c_int),
    "mgs_rasterize_bwd_det": ([i, p, p, p, p, p, p, i, i, i, i, i, p, p, p, p, p, p, p, p, p, u32, p, p, i, i, p, p, p, p, p, p, POINTER(c_size_t), p], c_int),
}
# every function include/mgs_optim.h declares (the same libraries; EXPORTS stays include/mgs.h's table)
_OPTIM_SIGNATURES = {
    "mgs_adam_step": ([i, POINTER(AdamGroup), c_double, c_double, c_double, p, p, p, i, c_size_t, p, p], c_int),
}
# every function include/mgs_refine.h declares (the same libraries again)
_REFINE_SIGNATURES = {
    "mgs_mcmc_weights": ([c_int64, p, f, i, p, p, p, p, POINTER(c_size_t), p], c_int),
    "mgs_mcmc_relocate": ([i, c_int64, c_int64, c_int64, p, p, i, POINTER(RefineGroup), f, p, p, p, p, p, p,
                           POINTER(c_size_t), p], c_int),
    "mgs_mcmc_noise": ([c_int64, p, p, p, p, p, c_double, c_double, c_double, c_int32, p, p], c_int),
}
# every function include/mgs_labels.h declares (the same libraries again): mgs_render_frames_labeled is
# mgs_render_frames with (class_ids, n_classes, labels, label_weights) in front of the workspace
_LABEL_SIGNATURES = {
    "mgs_raster_labels": ([i, p, p, p, p, p, i, i, i, i, i, p, p, p, p, p, p], c_int),
    "mgs_render_frames_labeled": (_SIGNATURES["mgs_render_frames"][0][:-3] + [p, i, p, p]
                                  + _SIGNATURES["mgs_render_frames"][0][-3:], c_int),
}
# every function include/mgs_lift.h declares (the same libraries again): votes are uint64 Q32 behind a void pointer
_LIFT_SIGNATURES = {
    "mgs_raster_votes": ([i, p, p, p, p, p, i, i, i, i, i, p, p, p, i, i, p, p], c_int),
    "mgs_lift_assign": ([i, i, p, f, p, p, p], c_int),
}
# every function include/mgs_hinge.h declares (the same libraries again): the workspace size is a query of its own, and
# joint is 16 doubles behind a void pointer
_HINGE_SIGNATURES = {
    "mgs_hinge_workspace_bytes": ([i, i], c_size_t),
    "mgs_hinge_fit": ([i, p, i, p, f, p, c_size_t, p, p, p, p], c_int),
}
# every function include/mgs_pose.h declares (the same libraries again): the workspace size is a query of its own, as the
# hinge's is; the four cotangents and the four rest-pose gradients are nullable
_POSE_SIGNATURES = {
    "mgs_pose_bwd_workspace_bytes": ([i, i], c_size_t),
    "mgs_pose_bwd": ([i, p, p, p, i, i, p, p, i, p, p, p, p, p, p, p, p, p, p, p, p, c_size_t, p], c_int),
}
# every function include/mgs_deform.h declares (the same libraries again): bind's workspace size is a query of its own, as
# the hinge's is; select and status are nullable
_DEFORM_SIGNATURES = {
    "mgs_deform_bind_workspace_bytes": ([i, i], c_size_t),
    "mgs_deform_bind": ([i, p, p, i, p, f, p, c_size_t, p, p, p, p, p, p], c_int),
    "mgs_deform_apply": ([i, p, p, p, p, p, p, p, p, i, i, p, p, p, p, p, p], c_int),
}
# every function include/mgs_deform_sh.h declares (the same libraries again): mgs_deform_apply's sixteen parameters, then
# (sh_degree, coeff_stride, sh_coeffs, out_sh, copy_unbound) in front of the stream
_DEFORM_SH_SIGNATURES = {
    "mgs_deform_apply_sh": (_DEFORM_SIGNATURES["mgs_deform_apply"][0][:-1] + [i, i, p, p, i, p], c_int),
}
# every function include/mgs_deform_bwd.h declares (the same libraries again): the workspace size is a query of its own; the
# three cotangents, the three rest gradients (as a set) and bwd_status are nullable
_DEFORM_BWD_SIGNATURES = {
    "mgs_deform_apply_bwd_workspace_bytes": ([i], c_size_t),
    "mgs_deform_apply_bwd": ([i, p, p, p, p, p, p, i, p, p, p, p, p, p, p, p, p, p, p, p, p, c_size_t, p], c_int),
}
# every function include/mgs_mesh.h declares (the same libraries again): the workspace size is a query of its own; link_ids,
# scales, the colours and normals are nullable
_MESH_SIGNATURES = {
    "mgs_mesh_workspace_bytes": ([i, i, i, i, i, POINTER(c_size_t)], c_int),
    "mgs_mesh_vertices": ([i, i, p, p, i, p, p, p, p, p, p], c_int),
    "mgs_mesh_raster": ([i, i, p, i, p, p, i, i, f, f, i, p, c_size_t, p], c_int),
    "mgs_mesh_resolve": ([i, i, p, i, p, p, p, p, i, i, i, f, p, c_size_t, p, p, p, p, p], c_int),
    "mgs_rasterize_mesh": ([i, i, p, p, i, p, p, p, p, p, i, p, p, p, i, i, f, f, i, i, f, p, c_size_t, p, p, p, p, p, p], c_int),
}
# every function include/mgs_mesh_texture.h declares (the same libraries again): the layout is a host-only query; wraps and
# descriptors of the layout call, the colours and normals are nullable
_MESH_TEXTURE_SIGNATURES = {
    "mgs_mesh_texture_layout": ([i, p, p, p, POINTER(c_size_t)], c_int),
    "mgs_mesh_build_mips": ([i, p, p, c_size_t, p], c_int),
    "mgs_mesh_resolve_textured": (_MESH_SIGNATURES["mgs_mesh_resolve"][0][:-1] + [p, p, i, p, p, c_size_t, i, p], c_int),
    "mgs_rasterize_mesh_textured": (_MESH_SIGNATURES["mgs_rasterize_mesh"][0][:-1] + [p, p, i, p, p, c_size_t, i, p], c_int),
}
# every function include/mgs_hybrid.h declares (the same libraries again): backdrop, tile_group_order and fg_visibility
# are nullable
_HYBRID_SIGNATURES = {
    "mgs_raster_over_opaque": ([i, p, p, p, p, i, p, p, p, p, p, p, i, i, i, i, p, p, p, p, p, p, p], c_int),
}
# every function include/mgs_mesh_lens.h declares (the same libraries again): mgs_mesh.h's raster, resolve and fused call
# with (camera_model, lens_rows) in place of Ks and (lens_workspace, lens_workspace_bytes) behind the workspace
_MESH_LENS_SIGNATURES = {
    "mgs_mesh_lens_workspace_bytes": ([i, i, i, POINTER(c_size_t)], c_int),
    "mgs_mesh_lens_rays": ([i, i, p, i, i, p, c_size_t, p], c_int),
    "mgs_mesh_raster_lens": ([i, i, p, i, p, i, p, i, i, f, f, i, p, c_size_t, p, c_size_t, p], c_int),
    "mgs_mesh_resolve_lens": ([i, i, p, i, p, p, p, i, p, i, i, i, f, p, c_size_t, p, c_size_t, p, p, p, p, p], c_int),
    "mgs_rasterize_mesh_lens": ([i, i, p, p, i, p, p, p, p, i, p, i, p, p, p, i, i, f, f, i, i, f, p, c_size_t, p, c_size_t,
                                 p, p, p, p, p, p], c_int),
}
# every function include/mgs_loss_rgbd.h declares (the same libraries again): (desc, render, target_rgb, target_depth, mask,
# ...) with target_depth, mask and terms nullable; each ends in (workspace, workspace_bytes, stream)
_RGBD_LOSS_SIGNATURES = {
    "mgs_rgbd_loss_fwd": ([POINTER(RgbdLoss), p, p, p, p, p, p, p, POINTER(c_size_t), p], c_int),
    "mgs_rgbd_loss_fwd_grad": ([POINTER(RgbdLoss), p, p, p, p, p, p, p, p, POINTER(c_size_t), p], c_int),
    "mgs_rgbd_loss_bwd": ([POINTER(RgbdLoss), p, p, p, p, p, p, p, POINTER(c_size_t), p], c_int),
}
# every function include/mgs_tsdf.h declares (the same libraries again): each starts with the volume; the count pass is its
# own size query (a null workspace), and the emit pass takes that workspace with its size by value
_TSDF_SIGNATURES = {
    "mgs_tsdf_integrate": ([POINTER(TsdfVolume), i, i, i, p, i, p, f, f, p, p, i, p], c_int),
    "mgs_tsdf_extract_count": ([POINTER(TsdfVolume), f, f, p, p, POINTER(c_size_t), p], c_int),
    "mgs_tsdf_extract_emit": ([POINTER(TsdfVolume), f, f, p, p, c_size_t, p, p, c_int64, p, c_int64, p, p], c_int),
}
# every function include/mgs_register.h declares (the same libraries again): the workspace size is a query of its own, as
# the hinge's is; init, correspondence, distance2 and history are nullable, result is 32 doubles behind a void pointer
_REGISTER_SIGNATURES = {
    "mgs_register_workspace_bytes": ([i, i, i], c_size_t),
    "mgs_register_icp": ([i, p, i, p, f, i, i, c_double, p, p, c_size_t, p, p, p, p, p], c_int),
}
del p, i, f, u32, img
# what _load binds: a new header adds its table here
_SIGNATURE_TABLES = (_SIGNATURES, _OPTIM_SIGNATURES, _REFINE_SIGNATURES, _LABEL_SIGNATURES, _LIFT_SIGNATURES,
                     _HINGE_SIGNATURES, _POSE_SIGNATURES, _DEFORM_SIGNATURES, _DEFORM_SH_SIGNATURES, _MESH_SIGNATURES,
                     _MESH_TEXTURE_SIGNATURES, _HYBRID_SIGNATURES, _DEFORM_BWD_SIGNATURES, _MESH_LENS_SIGNATURES,
                     _RGBD_LOSS_SIGNATURES, _TSDF_SIGNATURES, _REGISTER_SIGNATURES)
EXPORTS = list(_SIGNATURES)
OPTIM_EXPORTS = list(_OPTIM_SIGNATURES)
REFINE_EXPORTS = list(_REFINE_SIGNATURES)
LABEL_EXPORTS = list(_LABEL_SIGNATURES)
LIFT_EXPORTS = list(_LIFT_SIGNATURES)
HINGE_EXPORTS = list(_HINGE_SIGNATURES)
POSE_EXPORTS = list(_POSE_SIGNATURES)
DEFORM_EXPORTS = list(_DEFORM_SIGNATURES)
DEFORM_SH_EXPORTS = list(_DEFORM_SH_SIGNATURES)
DEFORM_BWD_EXPORTS = list(_DEFORM_BWD_SIGNATURES)
MESH_EXPORTS = list(_MESH_SIGNATURES)
HYBRID_EXPORTS = list(_HYBRID_SIGNATURES)
MESH_TEXTURE_EXPORTS = list(_MESH_TEXTURE_SIGNATURES)
MESH_LENS_EXPORTS = list(_MESH_LENS_SIGNATURES)
RGBD_LOSS_EXPORTS = list(_RGBD_LOSS_SIGNATURES)
TSDF_EXPORTS = list(_TSDF_SIGNATURES)
REGISTER_EXPORTS = list(_REGISTER_SIGNATURES)
MESH_LENS_NEWTON_STEPS, MESH_LENS_SUPERBLOCK = 12, 8   # MGS_MESH_LENS_NEWTON_STEPS, MGS_MESH_LENS_SUPERBLOCK
MESH_MAX_SIDE, MESH_LARGE_BLOCKS = 16368, 15   # MGS_MESH_MAX_SIDE, MGS_MESH_LARGE_BLOCKS
# MGS_MESH_TEXTURE_MAX_SIDE, MGS_MESH_MAX_TEXTURES, MGS_MESH_TEXTURE_DESC_WORDS, MGS_MESH_WRAP_*, MGS_MESH_FILTER_*
MESH_TEXTURE_MAX_SIDE, MESH_MAX_TEXTURES, MESH_TEXTURE_DESC_WORDS = 16384, 4096, 20
MESH_WRAP = {"repeat": 0, "clamp": 1, "mirror": 2}
MESH_FILTER = {"bilinear": 0, "trilinear": 1}
DEFORM_K = 8                                # MGS_DEFORM_K
LABEL_NONE, LABELS_MAX_CLASSES = 255, 32    # MGS_LABEL_NONE, MGS_LABELS_MAX_CLASSES


class MgsError(RuntimeError):
    pass


def _load(path: str = None, hooks: bool = False) -> ctypes.CDLL:
    LIB_PATH = path or globals()["LIB_PATH"]
    if not os.path.exists(LIB_PATH):
        raise MgsError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc); there is no "
            "CPU or PyTorch fallback for the render path.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.mgs_version.restype = c_int
    have = lib.mgs_version()
    if have != MGS_VERSION:      # shifted parameter lists would end in a GPU fault, not in an error
        raise MgsError(f"{LIB_PATH} reports ABI version {have}, this binding was written for {MGS_VERSION} "
                       "(include/mgs.h): rebuild the library (`python robosimgs_amd/csrc/build.py --force`)")
    for table in _SIGNATURE_TABLES:
        for name, (argtypes, restype) in table.items():
            fn = getattr(lib, name)          # AttributeError here == header/library mismatch
            fn.argtypes = argtypes
            fn.restype = restype
    if hooks:
        for name in DEBUG_HOOKS:
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = [c_int], None
        if os.environ.get("MGS_SORT_OPTS"):            # measurement knob: one-sweep radix passes (same lists)
            lib.mgs_debug_set_sort_opts(int(os.environ["MGS_SORT_OPTS"], 0))
        if os.environ.get("MGS_RASTER_OPTS"):          # measurement knob (scripts/, profiles/): never changes a pixel
            lib.mgs_debug_set_raster_opts(int(os.environ["MGS_RASTER_OPTS"], 0))
    return lib


_lib = None
_debug = None


def lib() -> ctypes.CDLL:
    """The library every op calls: libmgs.so, which has no process-global state.  MGS_USE_DEBUG_LIB=1 in the
    environment (measurement scripts that set MGS_SORT_OPTS / MGS_RASTER_OPTS) makes it libmgs_debug.so instead."""
    global _lib
    if _lib is None:
        _lib = debug_lib() if os.environ.get("MGS_USE_DEBUG_LIB") else _load()
    return _lib


def debug_lib() -> ctypes.CDLL:
    """libmgs_debug.so: the same sources with -DMGS_DEBUG_HOOKS, the only build that has mgs_debug_set_*."""
    global _debug
    if _debug is None:
        _debug = _load(DEBUG_LIB_PATH, hooks=True)
    return _debug


class use_debug_lib:
    """with use_debug_lib() as L: every op inside goes through libmgs_debug.so (tests of the hooks, A/B scripts)."""

    def __enter__(self):
        global _lib
        self._saved = _lib
        _lib = debug_lib()
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self._saved
        return False


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().mgs_last_error_string().decode("utf-8", "replace")
        raise MgsError(f"{what} failed with status {rc}: {msg}")


def ptr(t) -> int | None:
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_handle() -> int:
    return torch.cuda.current_stream().cuda_stream


_workspaces: dict = {}


def sized_call(fn, args, device, *, cached: bool, canary_bytes: int = 0, trailing=()):
    """Two-phase call of an entry point whose parameters end in (workspace, workspace_bytes, stream, *trailing): a size query (with a
    null workspace the call only reports the bytes it needs), then the call itself on a 256-byte aligned workspace of
    exactly that size, both on torch's current stream.  Each call site picks where the workspace comes from:
      cached=True   one growing scratch tensor per (device, stream, capturing): stream-ordered reuse is safe because
                    every consumer is enqueued on that stream, and once grown nothing is allocated;
      cached=False  a tensor of its own, released (stream-ordered) when the call returns.
    canary_bytes: a fresh workspace followed by that many 0xA5 bytes, returned so that a test can see nothing was
    written past the workspace.  Returns None otherwise."""
    stream, nbytes = stream_handle(), ctypes.c_size_t(0)
    check(fn(*args, None, ctypes.byref(nbytes), stream, *trailing), f"{fn.__name__}(size query)")
    size = nbytes.value
    if canary_bytes:
        buf = torch.full((size + 256 + canary_bytes,), 0xA5, dtype=torch.uint8, device=device)
    elif cached:
        key = (device.index, torch.cuda.current_stream(device).cuda_stream, torch.cuda.is_current_stream_capturing())
        buf = _workspaces.get(key)
        if buf is None or buf.numel() < size + 256:
            buf = _workspaces[key] = torch.empty(int((size + 256) * 1.25) + 256, dtype=torch.uint8, device=device)
    else:
        buf = torch.empty(size + 256, dtype=torch.uint8, device=device)
    pad = -buf.data_ptr() % 256
    check(fn(*args, buf.data_ptr() + pad, ctypes.byref(nbytes), stream, *trailing), fn.__name__)
    if canary_bytes:
        return buf[pad + size:pad + size + canary_bytes]


def require_device(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise MgsError("the render path runs on the GPU only: got a CPU tensor "
                           "(there is no CPU fallback; see oracle/ for the test-only checker)")


def check_tensor(name: str, t, dtype, shape, device=None) -> None:
    """The kernels read and write their arguments through raw pointers: `t` must be a contiguous tensor of `dtype` and
    `shape` (-1: any extent), on `device` where one is given, or the call ends here in a ValueError.  Attribute reads
    only: nothing is synchronised, allocated or launched."""
    if (isinstance(t, torch.Tensor) and t.dtype == dtype and t.dim() == len(shape) and t.is_contiguous()
            and all(s == -1 or s == d for s, d in zip(shape, t.shape)) and (device is None or t.device == device)):
        return
    want = (f"a contiguous {str(dtype)[6:]} tensor {list(shape)}" + (" (-1: any extent)" if -1 in shape else "")
            + ("" if device is None else f" on {device}"))
    got = type(t).__name__ if not isinstance(t, torch.Tensor) else (
        f"{'a' if t.is_contiguous() else 'a strided'} {str(t.dtype)[6:]} tensor {list(t.shape)} on {t.device}")
    raise ValueError(f"{name} must be {want}, got {got}")


def aligned_workspace(workspace, need: int, device):
    """A caller's workspace as the library takes it: (the uint8 tensor, the offset of its first 256-byte aligned byte);
    need + 256 bytes are allocated on `device` where none is given.  A given one is any contiguous uint8 tensor: whether it
    is large enough, 1-D or on that device is the call site's, or the library's, to say."""
    if workspace is None:
        workspace = torch.empty(need + 256, dtype=torch.uint8, device=device)
    elif not (isinstance(workspace, torch.Tensor) and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("workspace must be a contiguous uint8 tensor, got "
                         + (f"{workspace.dtype} with strides {workspace.stride()}" if isinstance(workspace, torch.Tensor)
                            else type(workspace).__name__))
    return workspace, -workspace.data_ptr() % 256
