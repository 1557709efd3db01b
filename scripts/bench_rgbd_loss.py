"""What the loss of a training step costs on the RGB+ED frame: the loss forward plus the gradient hand-over (backward with
unit_gradient, as Trainer.step does), HIP-event times, one process, every case warmed up first and the cases taken in
alternating rounds so that a drift of the machine falls on all of them alike.

  a  rgbd_loss(colors, target)                      unmasked, depth_lambda = 0: the four-channel frame read in place
  b  rgbd_loss(colors, target, depth, mask, 0.5)    float32 mask, depth term
  c  l1_ssim_loss(colors[..., :3], target)          the yardstick: a contiguous copy going in, autograd's pad coming out
  d  the loss of b composed in eager torch          torch.where masking, separable grouped conv2d, masked depth mean

Each case twice: called from Python as it stands ("eager": what the host enqueues between the two events counts), and
captured in a HIP graph and replayed ("graph": device time alone, the form bench.py's step runs in).
Prints one JSON line per case and mode (median and minimum over all rounds, and the per-round medians).
scripts/bench_rgbd_loss.py [--height H --width W --reps N --rounds R]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from robosimgs_amd import l1_ssim_loss, rgbd_loss, unit_gradient  # noqa: E402
from ssim_ref import C1, C2, window  # noqa: E402

DEV = "cuda"


def eager_window():
    """pytorch_msssim's separable window as the two grouped conv2d weights (made once: a capture cannot copy from the host)."""
    g = torch.from_numpy(window()).float().to(DEV)
    return g.view(1, 1, -1, 1).repeat(3, 1, 1, 1), g.view(1, 1, 1, -1).repeat(3, 1, 1, 1)


def eager_loss(colors, target, depth_t, mask, wh, ww, lam=0.2, lam_d=0.5):
    on, zero = (mask > 0)[..., None], torch.zeros((), device=colors.device)
    xm = torch.where(on, mask[..., None] * colors[..., :3], zero)
    ym = torch.where(on, mask[..., None] * target, zero)
    x, y = xm.permute(0, 3, 1, 2), ym.permute(0, 3, 1, 2)
    f = lambda t: torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, wh, groups=3), ww, groups=3)
    mx, my = f(x), f(y)
    vxx, vyy, vxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    s = (2 * mx * my + C1) * (2 * vxy + C2) / ((mx * mx + my * my + C1) * (vxx + vyy + C2))
    w = torch.where(torch.isfinite(depth_t) & (depth_t > 0), mask, zero)
    diff = torch.where(w > 0, colors[..., 3], zero) - torch.where(w > 0, depth_t, zero)
    return (1 - lam) * (xm - ym).abs().mean() + lam * (1 - s.mean()) + lam_d * (w * diff.abs()).sum() / w.sum()


def frame(h, w, seed=0):
    """colors [1, h, w, 4] (a leaf that wants a gradient), target, target_depth (5 % invalid), a blob mask (30 % zeros)."""
    gen = torch.Generator(DEV).manual_seed(seed)
    colors = torch.rand(1, h, w, 4, device=DEV, generator=gen)
    colors[..., 3] = 1.0 + 2.0 * colors[..., 3]
    target = torch.rand(1, h, w, 3, device=DEV, generator=gen)
    depth = 1.0 + 2.0 * torch.rand(1, h, w, device=DEV, generator=gen)
    depth[torch.rand(1, h, w, device=DEV, generator=gen) < 0.05] = 0.0
    coarse = torch.rand(1, (h + 15) // 16, (w + 15) // 16, device=DEV, generator=gen) >= 0.3
    mask = coarse.repeat_interleave(16, -2).repeat_interleave(16, -1)[..., :h, :w].float().contiguous()
    return colors.requires_grad_(True), target, depth, mask


def cases(colors, target, depth, mask):
    def run(loss_fn):
        def fn():
            colors.grad = None
            v = loss_fn()
            v.backward(gradient=unit_gradient(v))
        return fn
    wh, ww = eager_window()
    return {
        "a rgbd_loss unmasked": run(lambda: rgbd_loss(colors, target)),
        "b rgbd_loss mask + depth": run(lambda: rgbd_loss(colors, target, depth, mask, depth_lambda=0.5)),
        "c l1_ssim_loss(colors[..., :3])": run(lambda: l1_ssim_loss(colors[..., :3], target)),
        "d eager torch composition of b": run(lambda: eager_loss(colors, target, depth, mask, wh, ww)),
    }


def captured(fn):
    """fn captured in a HIP graph on a side stream (after one more warm call there): its replay."""
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.synchronize()
    return graph.replay


def event_times(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def measure(fns, reps, rounds, warmup=5):
    """{name: per-round lists of per-call ms}: every case warmed up, then `rounds` rounds over all cases in turn."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(event_times(fn, max(reps // 10, 3) if k.startswith("d") else reps))
    return out


def report(times, shape, **extra):
    for k, rounds in times.items():
        flat = [t for r in rounds for t in r]
        meds = [float(np.median(r)) for r in rounds]
        print(json.dumps({"case": k, "shape": list(shape), "ms_median": round(float(np.median(flat)), 4),
                          "ms_min": round(min(flat), 4), "round_medians_ms": [round(m, 4) for m in meds], **extra}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    colors, target, depth, mask = frame(a.height, a.width)
    fns = cases(colors, target, depth, mask)
    report(measure(fns, a.reps, a.rounds), colors.shape, mode="eager")
    report(measure({k: captured(fn) for k, fn in fns.items()}, a.reps, a.rounds), colors.shape, mode="graph")
