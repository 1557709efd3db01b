"""The fp64 torch oracle's run of examples/fit_joint_angle.py's descent, on the CPU: the trajectory recorded in
profiles/pose/README.md, which is what the constants THETA_0, THETA_STAR, LR, DECAY and STEPS of the example and the 1/4
of tests/test_gpu_pose.py::test_the_angle_of_the_lid_is_recovered rest on (the oracle has to end within 1/16).  The render
is oracle/gs_oracle_torch.render; the transform is written here in torch -- Rodrigues for the means, q_R (x) q with
q_R = (cos theta/2, sin theta/2 axis), the least-squares SH matrices of R(theta) -- and autograd differentiates all of it.
Needs no GPU and no libmgs.so; a few seconds.

    python scripts/pose_oracle_loop.py [lr decay steps]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gs_oracle_torch as OT  # noqa: E402
from robosimgs_amd.articulation import Hinge  # noqa: E402
from robosimgs_amd.gaussians import _sh_fit_basis  # noqa: E402
from robosimgs_amd.pose import _sh_basis_torch  # noqa: E402


def example():
    spec = importlib.util.spec_from_file_location("fit_joint_angle", os.path.join(ROOT, "examples", "fit_joint_angle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def main():
    E = example()
    lr, decay, steps = (float(sys.argv[1]), float(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (E.LR, E.DECAY, E.STEPS)
    W = H = 64
    scene, ids, edge, axis = E.lid_scene()              # the closed lid and the constructed hinge: the test's scene
    joint = np.zeros(16)
    joint[0:3], joint[3:6] = edge, axis
    hinge = Hinge(joint)
    cam = E.scene_camera(W, H)
    d = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    means, quats, scales, opac, colors = (d(a) for a in (scene.means, scene.quats, scene.scales, scene.opacities, scene.sh_coeffs))
    lid = torch.tensor(ids == E.LID)
    dirs, pinv = _sh_fit_basis(3)
    dirs, pinv = d(dirs), [d(p) for p in pinv]
    k = d(axis / np.linalg.norm(axis))

    def render(theta):
        R, t = hinge.pose_torch(theta)
        m = torch.where(lid[:, None], means @ R.T + t, means)
        q_r = torch.cat([torch.cos(theta / 2)[None], torch.sin(theta / 2) * k])
        q = torch.where(lid[:, None], quat_mul(q_r[None], quats), quats)
        Y = _sh_basis_torch(3, dirs @ R)
        parts = [colors[:, 0:1]]
        for l in (1, 2, 3):
            blk = slice(l * l, (l + 1) ** 2)
            parts.append(torch.einsum("ij,njc->nic", pinv[l] @ Y[:, blk], colors[:, blk]))
        c = torch.where(lid[:, None, None], torch.cat(parts, 1), colors)
        img, _alpha, _meta = OT.render(m, q, scales, opac, c, d(cam.viewmat()), d(cam.K), W, H, sh_degree=3)
        return img

    with torch.no_grad():
        target = render(torch.tensor(E.THETA_STAR, dtype=torch.float64))
    theta = torch.tensor(E.THETA_0, dtype=torch.float64, requires_grad=True)
    path = [E.THETA_0]
    for i in range(steps):
        loss = (render(theta) - target).abs().mean()
        theta.grad = None
        loss.backward()
        print(f"step {i:3d}  theta {path[-1]:+.5f}  L1 {float(loss.detach()):.5f}  dL/dtheta {float(theta.grad):+.5f}")
        with torch.no_grad():
            theta -= lr * decay ** i * theta.grad
        path.append(float(theta.detach()))
    print("trajectory: " + " ".join(f"{a:.5f}" for a in path))
    print(f"|theta_K - theta*| = {abs(path[-1] - E.THETA_STAR) / abs(E.THETA_0 - E.THETA_STAR):.4f} |theta_0 - theta*| "
          f"(lr {lr}, decay {decay}, {steps} steps)")


if __name__ == "__main__":
    main()
