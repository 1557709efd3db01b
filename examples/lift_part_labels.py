"""Part masks -> per-Gaussian part ids, as a round trip: a synthetic scene whose Gaussians carry known spatial classes is
rendered to label frames from a camera ring (the existing label path), and the label frames -- standing in for the 2D
segmentation masks a real capture would come with -- are lifted back onto the Gaussians with lift_labels.  Synthetic
inputs, so it runs anywhere an MI355X is visible:

    python examples/lift_part_labels.py [n_cameras]

The share of Gaussians that get their own class back is reported, not promised: a Gaussian's votes follow the majority
label of the pixels it is blended into, and at a pixel where two parts mix that is not always its own.
"""
import math
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from robosimgs_amd import camera_ring, lift_labels, rasterization, synthetic_scene  # noqa: E402


def main():
    n_cams = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    W, H, K = 640, 360, 4
    scene = synthetic_scene(100_000, math.log(0.02), 0, seed=0)
    t = scene.to_torch("cuda", 0)
    # known parts: an upper and a lower half, each cut once along world x
    m = t["means"]
    true = ((m[:, 2] > m[:, 2].median()).long() * 2 + (m[:, 0] > m[:, 0].median()).long()).to(torch.int32)
    cams = camera_ring(n_cams, W, H, radius=7.0)
    vm = torch.from_numpy(np.stack([c.viewmat() for c in cams]).astype(np.float32)).cuda()
    Ks = torch.from_numpy(np.stack([c.K for c in cams]).astype(np.float32)).cuda()
    args = (t["means"], t["quats"], t["scales"], t["opacities"])

    votes, chunk = None, 8                       # masks arrive in chunks, as they would from disk
    for c0 in range(0, n_cams, chunk):
        sl = slice(c0, min(c0 + chunk, n_cams))
        masks = rasterization(*args, t["colors"], vm[sl], Ks[sl], W, H, sh_degree=0, class_ids=true, n_classes=K)[2]["labels"]
        res = lift_labels(*args, vm[sl], Ks[sl], W, H, masks, K, votes=votes)
        votes = res.votes
    voted = res.class_ids >= 0
    same = (res.class_ids == true) & voted
    sure = voted & (res.confidence >= 0.9)
    print(f"{n_cams} label frames of {W}x{H}, {K} parts, {len(scene)} Gaussians")
    print(f"voted for by some pixel:            {int(voted.sum())} ({float(voted.float().mean()):.1%})")
    print(f"their own class back:               {float(same.sum()) / max(1, int(voted.sum())):.1%} of those")
    print(f"their own class back, conf >= 0.9:  {float((same & sure).sum()) / max(1, int(sure.sum())):.1%} of {int(sure.sum())}")
    # the result plugs straight back in: label frames from the lifted ids
    again = rasterization(*args, t["colors"], vm[:1], Ks[:1], W, H, sh_degree=0, class_ids=res.class_ids, n_classes=K)[2]["labels"]
    first = rasterization(*args, t["colors"], vm[:1], Ks[:1], W, H, sh_degree=0, class_ids=true, n_classes=K)[2]["labels"]
    print(f"label frame of camera 0 from the lifted ids: {float((again == first).float().mean()):.1%} of its pixels as rendered "
          "from the true ids")


if __name__ == "__main__":
    main()
