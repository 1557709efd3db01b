"""Where does the lid hinge?  A box of Gaussians with its lid standing open by 60 degrees, part ids per Gaussian (what
lift_labels returns on a real capture): fit_hinge finds the contact set of lid and body and the hinge line on the GPU,
and Hinge.pose(angle) is the transform FrameRenderer.submit takes for the lid's group -- the lid is then closed and opened
over a camera ring with no hard-coded joint anywhere.  Synthetic inputs, so it runs anywhere an MI355X is visible:

    python examples/fit_hinge.py [n_frames]
"""
import math
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from robosimgs_amd import FrameRenderer, camera_ring, fit_hinge  # noqa: E402
from robosimgs_amd.gaussians import Gaussians  # noqa: E402

BODY, LID = 0, 1


def sheet(origin, u, v, nu, nv, step):
    """nu x nv points origin + i step u + j step v."""
    i, j = [x.reshape(-1, 1) for x in np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")]
    return np.asarray(origin, np.float64) + step * (i * np.asarray(u, np.float64) + j * np.asarray(v, np.float64))


def main():
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    W, H, s = 960, 540, 0.02
    nx, ny, nz = 51, 31, 21                                    # a 1.0 x 0.6 x 0.4 box, open at the top
    body = np.concatenate([sheet((0, 0, 0), (1, 0, 0), (0, 1, 0), nx, ny, s),                   # floor
                           sheet((0, 0, 0), (1, 0, 0), (0, 0, 1), nx, nz, s), sheet((0, (ny - 1) * s, 0), (1, 0, 0), (0, 0, 1), nx, nz, s),
                           sheet((0, 0, 0), (0, 1, 0), (0, 0, 1), ny, nz, s), sheet(((nx - 1) * s, 0, 0), (0, 1, 0), (0, 0, 1), ny, nz, s)])
    open_by = math.radians(60.0)                               # the lid turns about the top edge of the wall y = 0
    lid = sheet((0, 0, (nz - 1) * s), (1, 0, 0), (0, math.cos(open_by), math.sin(open_by)), nx, ny, s)
    rng = np.random.default_rng(0)
    means = np.concatenate([body, lid]) + rng.uniform(-0.001, 0.001, (len(body) + len(lid), 3)) - [0.5, 0.3, 0.2]
    ids = np.concatenate([np.full(len(body), BODY), np.full(len(lid), LID)]).astype(np.int32)
    n = len(means)
    colour = np.where(ids[:, None] == LID, [0.9, 0.5, 0.1], [0.2, 0.4, 0.8]) + rng.uniform(-0.05, 0.05, (n, 3))
    scene = Gaussians(means, np.full((n, 3), math.log(0.012)), np.tile([1.0, 0, 0, 0], (n, 1)), np.full(n, 3.0),
                      (colour - 0.5) / 0.28209479177387814, np.zeros((n, 0, 3)))
    tensors = scene.to_torch("cuda", 0)
    class_ids = torch.from_numpy(ids).cuda()

    hinge = fit_hinge(tensors["means"], class_ids, part=LID, base=BODY, threshold=0.01)        # selection syncs: once per scene
    print(hinge)
    edge = np.array([0.0, -0.3, (nz - 1) * s - 0.2])
    off = hinge.position - edge
    print(f"constructed hinge: the line through {edge.tolist()} along x; fitted axis {math.degrees(math.acos(min(1.0, abs(hinge.axis[0])))):.2f} "
          f"degrees from it, position {np.linalg.norm(off - off[0] * np.array([1.0, 0, 0])):.4f} from the line")

    cams = camera_ring(n_frames, W, H, radius=2.2)
    group_ids = torch.where(class_ids == LID, 0, -1).to(torch.int32)
    r = FrameRenderer(tensors, W, H, render_mode="RGB", frames_in_flight=3, sizing_camera=(cams[0].viewmat(), cams[0].K),
                      capacity_margin=2.0, group_ids=group_ids, n_groups=1, labels=True)
    # the lid as built stands open by 60 degrees; angle 0 leaves it there, turning about the fitted axis closes and opens it
    sign = 1.0 if hinge.axis[0] > 0 else -1.0                  # the axis' sign is a convention (largest component positive)
    angles = -sign * open_by * 0.5 * (1 - np.cos(2 * np.pi * np.arange(n_frames) / n_frames))   # open -> closed -> open
    Rs, ts = hinge.pose(angles)
    lid_pixels, tickets, nxt = [], [], 0
    for i in range(n_frames):
        while nxt < n_frames and len(tickets) < r.n_slots:
            tickets.append(r.submit(cams[nxt].viewmat(), cams[nxt].K, rotations=[Rs[nxt]], translations=[ts[nxt]]))
            nxt += 1
        tk = tickets.pop(0)
        lid_pixels.append(int((r.fetch(tk)["labels"] == 1).sum()))
        r.release(tk)
    torch.cuda.synchronize()
    print(f"{n_frames} frames of {W}x{H} with the lid posed by Hinge.pose; lid pixels in the first / middle (closed) / last frame:",
          lid_pixels[0], lid_pixels[n_frames // 2], lid_pixels[-1])


if __name__ == "__main__":
    main()
