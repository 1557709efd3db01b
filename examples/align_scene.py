"""Bring a scene into the world frame.  A nerfstudio .ply lives in an arbitrary frame at an arbitrary scale; the robot and
the simulator live in a metric one.  Here a synthetic scene plays the world, a copy of it moved by a known similarity plays
the .ply, and samples of the original play the scanned target: register_points estimates the similarity from geometry alone
(ICP on the GPU, from a rough initial guess), Registration.apply moves the Gaussians, and the aligned scene is rendered from
the world's camera.  Synthetic inputs, so it runs anywhere an MI355X is visible:

    python examples/align_scene.py [n_gaussians]
"""
import math
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from robosimgs_amd import camera_ring, rasterization, register_points, synthetic_scene, transform_gaussians  # noqa: E402


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(degrees)
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def render(tensors, cam, W, H):
    vm = torch.from_numpy(cam.viewmat().astype(np.float32)).cuda()[None]
    K = torch.from_numpy(cam.K.astype(np.float32)).cuda()[None]
    img, _, _ = rasterization(tensors["means"], tensors["quats"], tensors["scales"], tensors["opacities"], tensors["colors"],
                              vm, K, W, H, sh_degree=tensors["sh_degree"])
    return img[0]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    W, H = 640, 480
    world = synthetic_scene(n, math.log(0.02), 1, 0).to_torch("cuda", 1)
    extent = float((world["means"].max(0).values - world["means"].min(0).values).max())

    # the .ply's frame: the world moved by the inverse of (R, t, s), which is what the registration has to find
    R, t, s = rotation([0.2, 1.0, 0.3], 12.0), np.array([0.04, -0.03, 0.05]) * extent, 1.6
    Ri, si = R.T, 1.0 / s
    ply = transform_gaussians(world, [Ri], [-si * Ri @ t], [si])

    # the target: every third mean of the world, jittered (a depth camera's cloud, or Mesh.sample_points of a scan)
    gen = torch.Generator(device="cuda").manual_seed(1)
    target = world["means"][::3] + 0.001 * extent * torch.randn(world["means"][::3].shape, device="cuda", generator=gen)

    # a rough guess (a few clicks in a viewer): 5 degrees, 1.5 % of the extent and 3 % of the scale off
    guess = (rotation([1.0, 0.0, 0.4], 5.0) @ R, t + 0.015 * extent, s * 1.03)
    reg = register_points(ply["means"], target, max_distance=0.05 * extent, init=guess, with_scale=True, iterations=40)
    print(reg)
    Re, te, se = reg.pose()
    angle = math.degrees(math.acos(min(1.0, (np.trace(Re @ R.T) - 1) / 2)))
    print(f"recovered against planted: rotation {angle:.4f} degrees, translation {np.abs(te - t).max() / extent:.2e} of the extent, "
          f"scale {se:.5f} (planted {s})")
    for k, (n_in, rmse, scale, _) in enumerate(reg.history):
        print(f"  iteration {k:2d}: {int(n_in)} inliers, rmse {rmse:.5f}, scale {scale:.5f}")

    aligned = reg.apply(ply)                                    # transform_gaussians with the estimated (R, t, s)
    cam = camera_ring(1, W, H, thetas=[0.4])[0]
    a, b = render(aligned, cam, W, H), render(world, cam, W, H)
    print(f"aligned scene against the world from one camera: mean |difference| {float((a - b).abs().mean()):.2e} "
          f"(before alignment {float((render(ply, cam, W, H) - b).abs().mean()):.2e})")


if __name__ == "__main__":
    main()
