"""At what angle does the lid stand?  A box of Gaussians whose lid turns about a hinge; a target image is rendered with the
lid opened by theta*, and from a start theta0 the angle descends on the L1 difference of the renders through

    Hinge.pose_torch(theta) -> pose_gaussians -> rasterization -> l1_loss

-- the pose gradient comes back through mgs_pose_bwd, one HIP pass over the Gaussians.  Synthetic inputs, so it runs
anywhere an MI355X is visible:

    python examples/fit_joint_angle.py [steps]
"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from robosimgs_amd.camera import Camera  # noqa: E402
from robosimgs_amd.gaussians import Gaussians  # noqa: E402

BODY, LID = 0, 1


def sheet(origin, u, v, nu, nv, step):
    """nu x nv points origin + i step u + j step v."""
    i, j = [x.reshape(-1, 1) for x in np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")]
    return np.asarray(origin, np.float64) + step * (i * np.asarray(u, np.float64) + j * np.asarray(v, np.float64))


def lid_scene(nx=10, ny=7, nz=4, step=0.1, sh_degree=3, seed=0, open_by=0.0):
    """An open-topped box of nx x ny x nz sheets of Gaussians and its lid, hinged on the top edge of the wall y = 0 and
    built standing open by `open_by` radians (0: lying closed on the box).  Returns (Gaussians, part ids int32 [N], a point
    of the hinge line, its axis)."""
    body = np.concatenate([sheet((0, 0, 0), (1, 0, 0), (0, 1, 0), nx, ny, step),
                           sheet((0, 0, 0), (1, 0, 0), (0, 0, 1), nx, nz, step),
                           sheet((0, (ny - 1) * step, 0), (1, 0, 0), (0, 0, 1), nx, nz, step),
                           sheet((0, 0, 0), (0, 1, 0), (0, 0, 1), ny, nz, step),
                           sheet(((nx - 1) * step, 0, 0), (0, 1, 0), (0, 0, 1), ny, nz, step)])
    lid = sheet((0, 0, (nz - 1) * step), (1, 0, 0), (0, np.cos(open_by), np.sin(open_by)), nx, ny, step)
    centre = np.array([(nx - 1) * step / 2, (ny - 1) * step / 2, (nz - 1) * step / 2])
    rng = np.random.default_rng(seed)
    n = len(body) + len(lid)
    means = np.concatenate([body, lid]) + rng.uniform(-0.1, 0.1, (n, 3)) * step - centre
    ids = np.concatenate([np.full(len(body), BODY), np.full(len(lid), LID)]).astype(np.int32)
    colour = np.where(ids[:, None] == LID, [0.9, 0.5, 0.1], [0.2, 0.4, 0.8]) + rng.uniform(-0.1, 0.1, (n, 3))
    quats = rng.normal(size=(n, 4))
    log_scales = np.log(step * rng.uniform(0.35, 0.7, (n, 3)))
    rest = rng.normal(0.0, 0.08, (n, (sh_degree + 1) ** 2 - 1, 3))
    scene = Gaussians(means, log_scales, quats, np.full(n, 2.0), (colour - 0.5) / 0.28209479177387814, rest)
    edge = np.array([0.0, 0.0, (nz - 1) * step]) - centre
    return scene, ids, edge, np.array([1.0, 0.0, 0.0])


def scene_camera(width=64, height=64):
    """A camera that sees the box from the front, above and to one side: the lid's opening changes the image."""
    return Camera.look_at((1.1, -1.5, 1.1), (0.0, 0.0, 0.1), (0.0, 0.0, 1.0), width, height, 50.0)


def render_posed(tensors, group_ids, hinge, theta, cam_t, width, height):
    """The image with the lid at `theta`: the differentiable path."""
    from robosimgs_amd import rasterization
    from robosimgs_amd.pose import pose_gaussians
    R, t = hinge.pose_torch(theta)
    posed = pose_gaussians(tensors, R[None], t[None], group_ids=group_ids)
    colors, _alphas, _meta = rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"],
                                           posed["colors"], cam_t[0], cam_t[1], width, height,
                                           sh_degree=tensors["sh_degree"])
    return colors


def fit_angle(tensors, group_ids, hinge, target, cam_t, width, height, theta0, lr, steps, decay=1.0, log=None):
    """Gradient descent of theta on l1_loss(render(theta), target) from theta0: step k moves by lr decay^k times the
    gradient (the gradient of an L1 loss keeps its size up to the minimum, so a fixed step would hop about it for ever).
    Returns the angles theta_0 .. theta_steps (floats)."""
    from robosimgs_amd import l1_loss
    theta = torch.tensor(float(theta0), dtype=torch.float64, device=tensors["means"].device, requires_grad=True)
    path = [float(theta0)]
    for k in range(steps):
        loss = l1_loss(render_posed(tensors, group_ids, hinge, theta, cam_t, width, height), target)
        theta.grad = None
        loss.backward()
        with torch.no_grad():
            theta -= lr * decay ** k * theta.grad
        path.append(float(theta.detach()))
        if log:
            log(k, path[-2], float(loss.detach()), float(theta.grad))
    return path


THETA_STAR, THETA_0 = 0.9, 0.4           # the lid stands open by 0.9 rad; the search starts at 0.4
LR, DECAY, STEPS = 4.0, 0.85, 24
BUILT_OPEN = 1.3                         # main(): the lid as built (only its hinge edge touches the box: fit_hinge finds it)


def main():
    from robosimgs_amd import fit_hinge
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else STEPS
    W = H = 64
    scene, ids, edge, axis = lid_scene(open_by=BUILT_OPEN)
    tensors = scene.to_torch("cuda", 3)
    class_ids = torch.from_numpy(ids).cuda()
    hinge = fit_hinge(tensors["means"], class_ids, part=LID, base=BODY, threshold=0.03)
    print(hinge)
    print(f"constructed hinge: the line through {edge.tolist()} along {axis.tolist()}")
    sign = 1.0 if hinge.axis[0] > 0 else -1.0                   # the axis' sign is a convention
    group_ids = torch.where(class_ids == LID, 0, -1).to(torch.int32)
    cam = scene_camera(W, H)
    cam_t = (torch.tensor(cam.viewmat()[None], dtype=torch.float32, device="cuda"),
             torch.tensor(cam.K[None], dtype=torch.float32, device="cuda"))
    # pose angles turn the lid from where it was built: opening theta is the pose angle sign * (theta - BUILT_OPEN)
    star, start = sign * (THETA_STAR - BUILT_OPEN), sign * (THETA_0 - BUILT_OPEN)
    with torch.no_grad():
        target = render_posed(tensors, group_ids, hinge, torch.tensor(star, dtype=torch.float64, device="cuda"), cam_t, W, H)
    print(f"target: the lid open by {THETA_STAR:.3f} rad (pose angle {star:+.3f}); start at {THETA_0:.3f} ({start:+.3f})")
    path = fit_angle(tensors, group_ids, hinge, target, cam_t, W, H, start, LR, steps, DECAY,
                     log=lambda k, th, loss, g: print(f"step {k:3d}  pose angle {th:+.4f}  L1 {loss:.5f}  dL/dtheta {g:+.5f}"))
    print(f"pose angle after {steps} steps: {path[-1]:+.4f} (target {star:+.4f}, "
          f"error {abs(path[-1] - star):.4f} of {abs(start - star):.4f} at the start)")


if __name__ == "__main__":
    main()
