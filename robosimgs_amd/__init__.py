"""robosimgs_amd -- MI355X-native 3D Gaussian Splatting render path for RoboSimGS scenes.

Host-side API (stays Python): Camera, Gaussians, load_ply / save_ply, synthetic_scene.
Device path (hand-written HIP for gfx950 behind the C ABI in include/mgs.h): the operators
in `ops` and `rasterization` / `render`.  Importing the device path needs torch and the
built libmgs.so; the host-side API needs only numpy.
"""
from .camera import (Camera, camera_ring, cameras_from_camera_params_json,
                     cameras_from_transforms_json, depth_to_distance, distance_to_depth,
                     unproject_point)
from .gaussians import (Gaussians, load_dataparser_transforms, load_ply, save_ply,
                        synthetic_scene, synthetic_scene_heavy_tailed)

__version__ = "0.1.0"

_DEVICE_API = {"rasterization", "render", "check_isect_status", "fully_fused_projection",
               "spherical_harmonics", "isect_tiles", "isect_offset_encode",
               "rasterize_to_pixels", "rasterize_labels", "rasterize_votes", "assign_classes", "lift_labels",
               "fit_hinge", "fit_hinge_points", "pose_gaussians", "bind_particles", "deform_gaussians",
               "deform_gaussians_autograd", "rasterize_mesh", "mesh_vertices", "mesh_raster", "mesh_resolve",
               "mesh_lens_rays", "render_sharded", "gather_frames", "TSDFVolume", "register_points"}


def __getattr__(name):  # lazy: keeps `import robosimgs_amd` torch-free for host-only use
    if name in ("rasterization", "render", "check_isect_status"):
        from . import rendering
        return getattr(rendering, name)
    if name in ("fully_fused_projection", "spherical_harmonics", "isect_tiles",
                "isect_offset_encode", "rasterize_to_pixels", "rasterize_labels", "rasterize_votes",
                "assign_classes"):
        from . import ops
        return getattr(ops, name)
    if name in ("lift_labels", "LiftResult"):
        from . import lifting
        return getattr(lifting, name)
    if name in ("fit_hinge", "fit_hinge_points", "hinge_fit_raw", "Hinge"):
        from . import articulation
        return getattr(articulation, name)
    if name in ("composite_over", "frame_to_u8"):
        from . import compositing
        return getattr(compositing, name)
    if name in ("frame_to_dataset", "DatasetWriter", "read_dataset_frame", "unnormalize_points"):
        from . import dataset
        return getattr(dataset, name)
    if name == "transform_gaussians":
        from . import transform
        return transform.transform_gaussians
    if name in ("pose_gaussians", "pack_transforms_torch", "pose_bwd_raw"):
        from . import pose
        return getattr(pose, name)
    if name in ("bind_particles", "deform_gaussians", "ParticleBinding", "deform_bind_raw", "deform_apply_raw",
                "deform_apply_sh_raw", "deform_gaussians_autograd", "deform_apply_bwd_raw"):
        from . import deform
        return getattr(deform, name)
    if name in ("Mesh", "Texture"):
        from . import mesh
        return getattr(mesh, name)
    if name in ("rasterize_mesh", "MeshRenderer", "mesh_vertices", "mesh_raster", "mesh_resolve", "mesh_workspace_bytes",
                "TextureSet", "build_texture_set", "mesh_lens_rays", "mesh_lens_workspace_bytes", "MeshLensMap"):
        from . import mesh_render
        return getattr(mesh_render, name)
    if name in ("l1_loss", "l1_ssim_loss", "ssim", "unit_gradient", "rgbd_loss"):
        from . import losses
        return getattr(losses, name)
    if name in ("TSDFVolume", "tsdf_integrate_raw", "tsdf_extract_raw", "check_extract_status"):
        from . import tsdf
        return getattr(tsdf, name)
    if name in ("register_points", "Registration", "register_icp_raw", "register_workspace"):
        from . import registration
        return getattr(registration, name)
    if name in ("FrameRenderer", "locality_order"):
        from . import pipeline
        return getattr(pipeline, name)
    if name in ("reorder_parameters", "Trainer"):
        from . import training
        return getattr(training, name)
    if name in ("GaussianAdam", "splatfacto_groups"):
        from . import optim
        return getattr(optim, name)
    if name == "MCMCStrategy":
        from . import strategy
        return strategy.MCMCStrategy
    if name in ("render_sharded", "gather_frames", "shard_cameras"):
        from . import distributed
        return getattr(distributed, name)
    raise AttributeError(name)
