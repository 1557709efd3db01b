"""What splatfacto's L1 + D-SSIM loss costs: HIP-event times, one process, warm-up first.

  1. l1_ssim_loss forward + gradient (the training form: the forward leaves the gradient, the backward with
     unit_gradient launches nothing) at 1920x1080x3 and 3840x2160x3, both paddings at 1080p;
  2. the same loss in eager torch (pytorch_msssim's separable grouped conv2d, autograd), same images;
  3. a Trainer step at 1 M Gaussians (synthetic_scene, RGB+ED, isect_capacity given, captured in a HIP graph as bench.py
     does) with l1_loss on all four channels (bench.py's step) and with l1_ssim_loss on colors[..., :3].
Prints one JSON line per measurement.  scripts/ssim_timing.py [--reps N]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from robosimgs_amd import Trainer, camera_ring, l1_loss, l1_ssim_loss, synthetic_scene, unit_gradient  # noqa: E402
from ssim_ref import C1, C2, window  # noqa: E402

DEV = "cuda"


def event_ms(fn, reps, warmup=5):
    """Median of per-call HIP-event times (ms) after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def torch_loss(render, target, lam=0.2):
    x, y = render.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)
    c = x.shape[1]
    g = torch.from_numpy(window()).float().to(render.device)
    wh, ww = g.view(1, 1, -1, 1).repeat(c, 1, 1, 1), g.view(1, 1, 1, -1).repeat(c, 1, 1, 1)
    f = lambda t: torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, wh, groups=c), ww, groups=c)
    mx, my = f(x), f(y)
    vxx, vyy, vxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    s = (2 * mx * my + C1) * (2 * vxy + C2) / ((mx * mx + my * my + C1) * (vxx + vyy + C2))
    return (1 - lam) * (render - target).abs().mean() + lam * (1 - s.mean())


def loss_times(reps):
    for (h, w), paddings in (((1080, 1920), ("valid", "same")), ((2160, 3840), ("valid",))):
        gen = torch.Generator(DEV).manual_seed(0)
        x = torch.rand(1, h, w, 3, device=DEV, generator=gen).requires_grad_(True)
        y = torch.rand(1, h, w, 3, device=DEV, generator=gen)
        for padding in paddings:
            def fused():
                x.grad = None
                v = l1_ssim_loss(x, y, 0.2, padding)
                v.backward(gradient=unit_gradient(v))
            med, best = event_ms(fused, reps)
            print(json.dumps({"what": "l1_ssim_loss fwd+grad (HIP)", "shape": [h, w, 3], "padding": padding,
                              "ms_median": round(med, 4), "ms_min": round(best, 4)}), flush=True)
            with torch.no_grad():
                med, best = event_ms(lambda: l1_ssim_loss(x, y, 0.2, padding), reps)
            print(json.dumps({"what": "l1_ssim_loss forward only (HIP)", "shape": [h, w, 3], "padding": padding,
                              "ms_median": round(med, 4), "ms_min": round(best, 4)}), flush=True)

        def eager():
            x.grad = None
            torch_loss(x, y).backward()
        med, best = event_ms(eager, reps)
        print(json.dumps({"what": "eager torch conv2d loss fwd+bwd", "shape": [h, w, 3], "padding": "valid",
                          "ms_median": round(med, 4), "ms_min": round(best, 4)}), flush=True)
        del x, y


def trainer_times(reps):
    n, W, H, deg = 1_000_000, 1920, 1080, 3
    g = synthetic_scene(n, math.log(0.012), deg, 0)
    cam = camera_ring(1, W, H, thetas=[0.3])[0]
    t = g.to_torch(DEV, deg)
    vm = torch.from_numpy(cam.viewmat().astype(np.float32)).to(DEV)[None]
    K = torch.from_numpy(cam.K.astype(np.float32)).to(DEV)[None]
    target = torch.rand(1, H, W, 4, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    for name, loss_fn in (("l1_loss (RGB+ED, 4 channels)", lambda c: l1_loss(c, target)),
                          ("l1_ssim_loss (colors[..., :3])", lambda c: l1_ssim_loss(c[..., :3], target[..., :3]))):
        params = {k: t[k].detach().clone().requires_grad_(True) for k in Trainer.KEYS}
        tr = Trainer(params, None, W, H, auto_reorder_every=0, sh_degree=deg, render_mode="RGB+ED", isect_capacity=4_700_000)

        def step():
            for p in params.values():
                p.grad = None
            colors, _, _ = tr.render(vm, K)
            tr.step(loss_fn(colors))

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        side = torch.cuda.Stream(DEV)
        with torch.cuda.stream(side):
            step()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                step()
        torch.cuda.synchronize()
        med, best = event_ms(graph.replay, reps)
        print(json.dumps({"what": "Trainer step, 1M Gaussians, 1920x1080, HIP graph", "loss": name,
                          "ms_median": round(med, 4), "ms_min": round(best, 4)}), flush=True)
        del graph, tr, params


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    loss_times(a.reps)
    trainer_times(a.reps)
