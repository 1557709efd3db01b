"""Train a background against RGB-D captures that have something in the way.  A synthetic scene is rendered from a ring of
cameras (colour and expected depth: the targets); into every target an occluder is pasted at the same place of the image
-- the arm that rides along with the camera -- in colour and, nearer than the scene, in depth.  From a start with grey
colours and jittered positions the scene is then trained twice through

    Trainer.render (RGB+ED) -> rgbd_loss(colors, target_rgb, target_depth, mask, depth_lambda) -> Trainer.step

once with the occluder masked out and once without a mask.  The occluder hides a different part of the scene in each view,
so the unmasked run paints it onto Gaussians that the other views see in the open; the PSNR against the clean renders,
taken OUTSIDE the occluder, says how much that costs.  Synthetic inputs, so it runs anywhere an MI355X is visible:

    python examples/train_masked_rgbd.py [steps]
"""
import math
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

W, H, N, SH_DEGREE, CAMERAS, STEPS = 256, 192, 20_000, 1, 6, 240
BOX = (slice(50, 140), slice(70, 180))            # the occluder's rows and columns in every view
DEV = "cuda"


def psnr_outside(render_rgb, clean_rgb, mask):
    """PSNR (data range 1) over the pixels where mask == 1."""
    mse = (((render_rgb - clean_rgb) ** 2).mean(-1) * mask).sum() / mask.sum()
    return float(-10.0 * torch.log10(mse))


def train(start, views, use_mask, steps):
    """`steps` steps of Adam on a copy of `start`, one view per step in turn.  Returns the trained parameters."""
    from robosimgs_amd import Trainer, rgbd_loss
    params = {k: start[k].detach().clone().requires_grad_(True) for k in Trainer.KEYS}
    lrs = {"means": 2e-4, "quats": 0.0, "scales": 0.0, "opacities": 0.0, "colors": 1e-2}   # colour and position train
    opt = torch.optim.Adam([{"params": [params[k]], "lr": lr} for k, lr in lrs.items()])
    tr = Trainer(params, opt, W, H, auto_reorder_every=0, sh_degree=SH_DEGREE, render_mode="RGB+ED")
    for it in range(steps):
        vm, K, rgb, depth, mask = views[it % len(views)]
        colors, _alphas, _meta = tr.render(vm, K)
        loss, terms = rgbd_loss(colors, rgb, depth, mask if use_mask else None, ssim_lambda=0.2, depth_lambda=0.5,
                                return_terms=True)
        tr.step(loss)
        if it % 60 == 0 or it == steps - 1:
            l1, ssim, d, sw = terms.tolist()
            print(f"  step {it:4d}  loss {float(loss.detach()):.4f}  mean|x-y| {l1:.4f}  ssim {ssim:.4f}  depth L1 {d:.4f}  "
                  f"(weight {sw:.0f} px)")
    return params


def main():
    from robosimgs_amd import camera_ring, rasterization, synthetic_scene
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else STEPS
    torch.cuda.set_device(0)
    truth = synthetic_scene(N, math.log(0.03), SH_DEGREE, 0).to_torch(DEV, SH_DEGREE)

    def render(p, vm, K):
        with torch.no_grad():
            return rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], vm, K, W, H,
                                 sh_degree=SH_DEGREE, render_mode="RGB+ED")[0]

    mask = torch.ones(1, H, W, device=DEV)
    mask[:, BOX[0], BOX[1]] = 0.0                 # float32, made once and kept on the device
    views, clean = [], []
    for cam in camera_ring(CAMERAS, W, H):
        vm = torch.from_numpy(cam.viewmat().astype(np.float32)).to(DEV)[None]
        K = torch.from_numpy(cam.K.astype(np.float32)).to(DEV)[None]
        frame = render(truth, vm, K)
        clean.append(frame[..., :3].clone())
        rgb, depth = frame[..., :3].clone(), frame[..., 3].clone()
        rgb[:, BOX[0], BOX[1]] = torch.tensor([0.9, 0.1, 0.6], device=DEV)       # the arm: one colour, ...
        near = depth[depth > 0].min() if bool((depth > 0).any()) else torch.tensor(1.0, device=DEV)
        depth[:, BOX[0], BOX[1]] = 0.5 * near                                    # ... in front of everything
        views.append((vm, K, rgb, depth, mask))

    gen = torch.Generator(DEV).manual_seed(1)
    start = {k: v.clone() if torch.is_tensor(v) else v for k, v in truth.items()}
    start["colors"] = torch.zeros_like(truth["colors"])                          # grey, no view dependence
    start["means"] = truth["means"] + 0.01 * torch.randn(truth["means"].shape, device=DEV, generator=gen)

    def score(p):
        return float(np.mean([psnr_outside(render(p, vm, K)[..., :3], c, mask) for (vm, K, *_), c in zip(views, clean)]))

    print(f"{N} Gaussians, {CAMERAS} views of {W} x {H}, occluder {BOX[1].stop - BOX[1].start} x {BOX[0].stop - BOX[0].start} px "
          f"({100 * float(1 - mask.mean()):.0f} % of each view), {steps} steps")
    print(f"PSNR outside the occluder at the start: {score(start):.2f} dB")
    results = {}
    for use_mask in (True, False):
        print("with the mask:" if use_mask else "without a mask:")
        results[use_mask] = score(train(start, views, use_mask, steps))
    print(f"PSNR outside the occluder, trained with the mask:  {results[True]:.2f} dB")
    print(f"PSNR outside the occluder, trained without a mask: {results[False]:.2f} dB")


if __name__ == "__main__":
    main()
