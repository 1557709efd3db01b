"""From a Gaussian scene to the triangle mesh a physics simulator collides with.

    python examples/extract_collision_mesh.py --out background.obj                  # a synthetic table-top scene
    python examples/extract_collision_mesh.py --ply scene.ply --lo -2 -2 0 --hi 2 2 2 --voxel 0.02 --out background.obj
    python examples/extract_collision_mesh.py --check                               # and compare with a held-out view

The scene (a nerfstudio / 3DGS .ply, or a plane with a sphere on it made of flat opaque Gaussians) is rendered from a ring of
cameras with rasterization(render_mode="RGB+ED"); the frames' expected depth is fused into a TSDFVolume over the box lo .. hi
(one launch for all views), the isosurface is extracted on the GPU and written as an .obj with vertex colours, which
Mesh.from_obj and rasterize_mesh take back.  --check rasterises that mesh from a camera the volume never saw and prints how
far its depth is from the splat frame's expected depth at the pixels both cover."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from robosimgs_amd import Camera, Mesh, TSDFVolume, load_ply, rasterization, rasterize_mesh  # noqa: E402

DEV = "cuda"


def surfel_scene():
    """rasterization's first five arguments for about 3,000 flat opaque Gaussians: a table top z = 0.3 and a ball on it."""
    g = np.arange(-0.5, 1.7001, 0.05)
    px, py = np.meshgrid(g, g)
    plane = np.stack([px.ravel(), py.ravel(), np.full(px.size, 0.3)], 1)
    k = np.arange(1000) + 0.5
    phi, z = np.pi * (1 + 5 ** 0.5) * k, 1 - 2 * k / 1000
    n_ball = np.stack([np.cos(phi) * np.sqrt(1 - z * z), np.sin(phi) * np.sqrt(1 - z * z), z], 1)
    normals = np.concatenate([np.tile([0.0, 0.0, 1.0], (len(plane), 1)), n_ball])
    quats = np.stack([1 + normals[:, 2], -normals[:, 1], normals[:, 0], np.zeros(len(normals))], 1)     # z axis -> normal (wxyz)
    quats[quats[:, 0] < 1e-6] = [0.0, 1.0, 0.0, 0.0]
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    means = np.concatenate([plane, np.array([0.6, 0.6, 0.52]) + 0.22 * n_ball])
    scales = np.concatenate([np.tile([0.035, 0.035, 0.002], (len(plane), 1)), np.tile([0.02, 0.02, 0.002], (1000, 1))])
    colors = np.concatenate([np.tile([0.55, 0.4, 0.25], (len(plane), 1)), np.tile([0.8, 0.25, 0.2], (1000, 1))])
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)
    return (f32(means), f32(quats), f32(scales), torch.full((len(means),), 0.99, device=DEV), f32(colors)), {}


def ring(n, centre, radius, height, width, img_height, fov, phase=0.0):
    cams = [Camera.look_at((centre[0] + radius * math.cos(t), centre[1] + radius * math.sin(t), centre[2] + height), tuple(centre),
                           (0.0, 0.0, 1.0), width, img_height, fov) for t in (phase + 2 * math.pi * k / n for k in range(n))]
    vm = torch.from_numpy(np.stack([c.viewmat() for c in cams]).astype(np.float32)).to(DEV)
    Ks = torch.from_numpy(np.stack([c.K for c in cams]).astype(np.float32)).to(DEV)
    return vm, Ks


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ply", help="a 3DGS .ply; default: the synthetic table-top scene")
    ap.add_argument("--lo", type=float, nargs=3, default=[0.0, 0.0, 0.0], help="low corner of the fused box")
    ap.add_argument("--hi", type=float, nargs=3, default=[1.2, 1.2, 1.2], help="high corner of the fused box")
    ap.add_argument("--voxel", type=float, default=0.0125)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--fov", type=float, default=60.0, help="horizontal field of view of the ring's cameras, degrees")
    ap.add_argument("--out", default="collision_mesh.obj")
    ap.add_argument("--check", action="store_true", help="compare the mesh with the splat frame from a held-out camera")
    a = ap.parse_args()
    torch.cuda.set_device(0)

    if a.ply:
        t = load_ply(a.ply).to_torch(DEV)
        scene, kw = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"]), dict(sh_degree=t["sh_degree"])
    else:
        scene, kw = surfel_scene()
    lo, hi = np.asarray(a.lo), np.asarray(a.hi)
    centre, size = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    vm, Ks = ring(a.views, centre, 0.9 * size, 0.45 * size, a.width, a.height, a.fov)
    frames, alphas, _ = rasterization(*scene, vm, Ks, a.width, a.height, render_mode="RGB+ED", **kw)

    vol = TSDFVolume.from_bounds(lo, hi, a.voxel, device=DEV)
    vol.integrate(frames, vm, Ks, alphas=alphas)                 # one launch: the volume is read and written once
    mesh = vol.extract_mesh()
    mesh.to_obj(a.out)
    print(f"{a.views} views of {a.width} x {a.height} into {vol.dims[0]} x {vol.dims[1]} x {vol.dims[2]} samples of {a.voxel} -> "
          f"{mesh.n_vertices} vertices, {mesh.n_faces} faces -> {a.out}")

    back = Mesh.from_obj(a.out).to(DEV)                          # what a simulator's importer would read
    assert back.n_faces == mesh.n_faces and torch.equal(back.vertices, mesh.vertices)
    if a.check:
        vm_h, K_h = ring(1, centre, 0.8 * size, 0.55 * size, a.width, a.height, a.fov, phase=math.pi / a.views)
        held, held_alpha, _ = rasterization(*scene, vm_h, K_h, a.width, a.height, render_mode="RGB+ED", **kw)
        _, depth, meta = rasterize_mesh(back, vm_h, K_h, a.width, a.height)
        both = (meta["face_ids"][0] >= 0) & (held_alpha[0, ..., 0] > 0.5)
        err = (depth[0] - held[0, ..., 3]).abs()[both]
        print(f"held-out camera: {int(both.sum())} pixels covered by both; |mesh depth - expected depth| median "
              f"{float(err.median()):.5f} ({float(err.median()) / a.voxel:.2f} voxel), 90th percentile "
              f"{float(err.quantile(0.9)):.5f}")
