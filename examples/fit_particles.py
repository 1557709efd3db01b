"""How high is the wave, and where is it?  A sheet of cloth, Gaussians bound to a grid of particles; a target image is
rendered with the particles on a wave z = A* sin(3 x + phi*), and from a start (A0, phi0) Adam descends on the L1 difference
of the renders through

    wave(A, phi) in torch -> deform_gaussians_autograd -> rasterization -> l1_loss

-- the particles' gradient comes back through mgs_deform_apply_bwd (two HIP launches, no float atomics) and torch carries
it on into the two parameters that made the positions: system identification through the renderer.  --per-particle fits
the positions themselves instead (every particle's z, from the flat sheet).  Synthetic inputs, so it runs anywhere an
MI355X is visible; it prints the trajectory and is a demonstration, not a gate:

    python examples/fit_particles.py [--steps 150] [--per-particle]
"""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

A_STAR, PHI_STAR = 0.15, 0.7             # the wave in the target frame
A_0, PHI_0 = 0.05, 0.2                   # where the search starts
W = H = 64


def cloth_scene(n_side=18, m_side=12, device="cuda"):
    """A sheet of n_side^2 Gaussians over a grid of m_side^2 particles in front of a 64 x 64 camera (the shapes of the
    deformation tests' cloth): (tensors, particles [M,3], viewmat [1,4,4], K [1,3,3])."""
    rng = np.random.default_rng(8)
    gx, gy = np.meshgrid(np.linspace(-0.8, 0.8, n_side), np.linspace(-0.8, 0.8, n_side), indexing="ij")
    means = np.stack([gx.reshape(-1), gy.reshape(-1), 0.01 * rng.normal(size=n_side * n_side)], 1)
    n = len(means)
    px, py = np.meshgrid(np.linspace(-0.9, 0.9, m_side), np.linspace(-0.9, 0.9, m_side), indexing="ij")
    parts = np.stack([px.reshape(-1), py.reshape(-1), np.zeros(m_side * m_side)], 1)
    quats = rng.normal(size=(n, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=device)
    tensors = dict(means=t(means), quats=t(quats), scales=t(np.exp(rng.uniform(-3.2, -2.6, (n, 3)))),
                   opacities=t(rng.uniform(0.3, 0.9, n)), colors=t(rng.uniform(0, 1, (n, 1, 3))), sh_degree=0)
    vm = np.eye(4)
    vm[2, 3] = 2.5
    K = np.array([[60.0, 0, 32], [0, 60.0, 32], [0, 0, 1]])
    return tensors, t(parts), t(vm)[None], t(K)[None]


def wave(parts, amplitude, phase):
    """The particles on the wave z = amplitude sin(3 x + phase), in torch: autograd sees the two parameters."""
    z = amplitude * torch.sin(3.0 * parts[:, 0] + phase)
    return torch.stack([parts[:, 0], parts[:, 1], z.to(parts.dtype)], 1)


def render(tensors, binding, particles, vm, K):
    from robosimgs_amd import deform_gaussians_autograd, rasterization
    posed = deform_gaussians_autograd(tensors, binding, particles)
    colors, _alphas, _meta = rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"],
                                           posed["colors"], vm, K, W, H, sh_degree=0)
    return colors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--per-particle", action="store_true", help="fit every particle's height instead of the wave's two parameters")
    a = ap.parse_args()
    from robosimgs_amd import bind_particles, l1_loss
    tensors, parts, vm, K = cloth_scene()
    binding = bind_particles(tensors["means"], parts)
    star = wave(parts, torch.tensor(A_STAR, device="cuda"), torch.tensor(PHI_STAR, device="cuda"))
    with torch.no_grad():
        target = render(tensors, binding, star, vm, K)
    if a.per_particle:
        z = torch.zeros(parts.shape[0], device="cuda", requires_grad=True)
        params, lr = [z], 0.01
        positions = lambda: torch.stack([parts[:, 0], parts[:, 1], z], 1)
        report = lambda: f"rms height error {float((z.detach() - star[:, 2]).square().mean().sqrt()):.4f}"
        print(f"target: the wave {A_STAR} sin(3 x + {PHI_STAR}); start: the flat sheet ({report()})")
    else:
        amp = torch.tensor(A_0, dtype=torch.float64, device="cuda", requires_grad=True)
        phi = torch.tensor(PHI_0, dtype=torch.float64, device="cuda", requires_grad=True)
        params, lr = [amp, phi], 0.02
        positions = lambda: wave(parts, amp, phi)
        report = lambda: f"amplitude {float(amp.detach()):+.4f}  phase {float(phi.detach()):+.4f}"
        print(f"target: amplitude {A_STAR:+.4f}  phase {PHI_STAR:+.4f}; start: {report()}")
    opt = torch.optim.Adam(params, lr=lr)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.985)     # an L1 gradient keeps its size up to the minimum
    for k in range(a.steps):
        opt.zero_grad(set_to_none=True)
        loss = l1_loss(render(tensors, binding, positions(), vm, K), target)
        loss.backward()
        opt.step()
        sched.step()
        if k % 10 == 0 or k == a.steps - 1:
            print(f"step {k:4d}  L1 {float(loss.detach()):.5f}  {report()}")
    if not a.per_particle:
        print(f"after {a.steps} steps: {report()} (target amplitude {A_STAR:+.4f}  phase {PHI_STAR:+.4f})")


if __name__ == "__main__":
    main()
