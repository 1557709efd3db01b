"""A sheet of cloth that follows simulated particles.  A sheet of Gaussians is bound once to a coarser grid of particles
(bind_particles: 8 nearest particles per Gaussian, on the GPU), then a travelling wave computed in torch moves the
particles -- no simulator needed -- and FrameRenderer(deform=binding) deforms the Gaussians inside every frame's graph:
a submit uploads one [M,3] tensor.  A rigid block beside the sheet stays unbound (max_distance).  Synthetic inputs, so
it runs anywhere an MI355X is visible:

    python examples/deform_cloth.py [n_frames] [rigid|affine] [--rotate-sh]

--rotate-sh: the sheet gets degree-3 SH (a view-dependent sheen) and FrameRenderer(deform_rotate_sh=True) turns every
Gaussian's SH rows with it; a second renderer without the rotation renders the same frames, and the difference between the
two images is printed: the sheen that stayed in the world frame where the cloth turned.
"""
import math
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from robosimgs_amd import FrameRenderer, bind_particles, camera_ring  # noqa: E402
from robosimgs_amd.deform import STATUS_FALLBACK, STATUS_NONFINITE, STATUS_THIN, STATUS_UNBOUND  # noqa: E402
from robosimgs_amd.gaussians import Gaussians  # noqa: E402


def main():
    rotate_sh = "--rotate-sh" in sys.argv
    argv = [a for a in sys.argv[1:] if a != "--rotate-sh"]
    n_frames = int(argv[0]) if len(argv) > 0 else 48
    mode = argv[1] if len(argv) > 1 else "rigid"
    W, H = 960, 540
    rng = np.random.default_rng(0)
    ns, ms = 160, 48                                           # 160 x 160 Gaussians over 48 x 48 particles, 1.6 x 1.6
    gx, gy = np.meshgrid(np.linspace(-0.8, 0.8, ns), np.linspace(-0.8, 0.8, ns), indexing="ij")
    sheet = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(ns * ns)], 1) + rng.uniform(-0.002, 0.002, (ns * ns, 3))
    block = rng.uniform(-0.1, 0.1, (2000, 3)) + [0.0, 0.0, -0.6]                               # not cloth: stays where it is
    means = np.concatenate([sheet, block])
    n = len(means)
    stripes = (np.floor(means[:, 0] * 5) + np.floor(means[:, 1] * 5)) % 2
    colour = np.where(stripes[:, None] > 0, [0.85, 0.2, 0.2], [0.95, 0.9, 0.8]) + rng.uniform(-0.03, 0.03, (n, 3))
    scene = Gaussians(means, np.tile(np.log([0.008, 0.008, 0.002]), (n, 1)), np.tile([1.0, 0, 0, 0], (n, 1)), np.full(n, 3.0),
                      (colour - 0.5) / 0.28209479177387814,
                      rng.normal(0.0, 0.12, (n, 15, 3)) if rotate_sh else np.zeros((n, 0, 3)))
    tensors = scene.to_torch("cuda", 3 if rotate_sh else 0)

    px, py = torch.meshgrid(torch.linspace(-0.85, 0.85, ms), torch.linspace(-0.85, 0.85, ms), indexing="ij")
    rest = torch.stack([px.reshape(-1), py.reshape(-1), torch.zeros(ms * ms)], 1).cuda()
    binding = bind_particles(tensors["means"], rest, max_distance=0.1)          # once per object
    print(f"{binding.n_bound()} of {n} Gaussians bound to {binding.m} particles")

    cams = camera_ring(n_frames, W, H, radius=2.4)
    r = FrameRenderer(tensors, W, H, render_mode="RGB", frames_in_flight=3, sizing_camera=(cams[0].viewmat(), cams[0].K),
                      capacity_margin=2.5, deform=binding, deform_mode=mode, deform_rotate_sh=rotate_sh)
    unturned = FrameRenderer(tensors, W, H, render_mode="RGB", frames_in_flight=1, sizing_camera=(cams[0].viewmat(), cams[0].K),
                             capacity_margin=2.5, deform=binding, deform_mode=mode) if rotate_sh else None

    def particles_at(k):                                       # a travelling wave across the sheet, on the device
        phase = 2 * math.pi * k / n_frames
        x = rest.clone()
        x[:, 2] = 0.12 * torch.sin(4.0 * rest[:, 0] + phase) * (0.5 + 0.5 * torch.cos(2.0 * rest[:, 1]))
        x[:, 0] = rest[:, 0] * (1.0 - 0.05 * math.sin(phase))
        return x

    counts = np.zeros(5, np.int64)                             # ok, unbound, fell back to rigid, thin, non-finite
    covered, tickets, nxt, diffs = [], [], 0, []
    for _ in range(n_frames):
        while nxt < n_frames and len(tickets) < r.n_slots:
            tickets.append(r.submit(cams[nxt].viewmat(), cams[nxt].K, particles=particles_at(nxt)))
            nxt += 1
        tk = tickets.pop(0)
        f = r.fetch(tk)
        st = f["deform_status"]
        counts += np.array([int((st == 0).sum()), int((st & STATUS_UNBOUND != 0).sum()), int((st & STATUS_FALLBACK != 0).sum()),
                            int((st & STATUS_THIN != 0).sum()), int((st & STATUS_NONFINITE != 0).sum())])
        covered.append(float((f["colors"].sum(-1) > 0.05).float().mean()))
        if unturned is not None:                               # the same frame with the SH rows left in the world frame
            k = len(covered) - 1
            tk0 = unturned.submit(cams[k].viewmat(), cams[k].K, particles=particles_at(k))
            d = (f["colors"] - unturned.fetch(tk0)["colors"]).abs()
            diffs.append((float(d.mean()), float(d.max()), float((d.amax(-1) > 1.0 / 255).float().mean())))
            unturned.release(tk0)
        r.release(tk)
    torch.cuda.synchronize()
    share = 100.0 * counts / (n * n_frames)
    print(f"{n_frames} frames of {W}x{H} rendered with the {mode} deformation; covered pixels in the first / middle / last frame: "
          f"{covered[0]:.3f} {covered[n_frames // 2]:.3f} {covered[-1]:.3f}")
    print(f"status per Gaussian and frame: deformed {share[0]:.2f} %, unbound {share[1]:.2f} %, affine fell back to rigid "
          f"{share[2]:.2f} %, thin (translated only) {share[3]:.2f} %, non-finite neighbour {share[4]:.2f} %")
    if diffs:
        d = np.array(diffs)
        print(f"SH rows turned with the cloth against left in the world frame, per frame: mean |difference| {d[:, 0].mean():.4f} "
              f"(worst frame {d[:, 0].max():.4f}), largest {d[:, 1].max():.3f}, pixels off by more than 1/255: {100 * d[:, 2].mean():.1f} %")


if __name__ == "__main__":
    main()
