"""What the raw parameter form (rasterization(raw_params=True)) costs and saves in a training step: HIP-event times of
three variants of the Trainer step at BASELINE configs[2]'s shape (1 M Gaussians, SH 3, 1920x1080, "RGB+ED", L1, one HIP
graph each, the Trainer's Morton order), ALTERNATED within one process so that drift hits all three alike:

  (a) activated leaves, no activation ops   -- the step bench.py times
  (b) raw leaves through torch.exp / torch.sigmoid into the activated path   -- what a trainer runs today
  (c) raw leaves with raw_params=True       -- the activations fused into the projection kernels

Prints one JSON line per variant (median, min, 5th / 95th percentile) and one with the differences.  --variant a|b|c replays that variant's graph alone --reps times after the warm-up: the form to put under
`rocprofv3 --kernel-trace --stats -- python scripts/raw_params_timing.py --variant c --reps 20` for kernel names, call
counts and the project_color_fwd / _bwd kernel times.

scripts/raw_params_timing.py [--reps N] [--variant a|b|c]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from robosimgs_amd import Trainer, camera_ring, l1_loss, synthetic_scene  # noqa: E402

DEV = "cuda"
N, W, H, DEG, CAP = 1_000_000, 1920, 1080, 3, 4_700_000


def build(variant, g, vm, K, target):
    """The captured step of one variant: (graph, things to keep alive)."""
    raw = variant in ("b", "c")
    t = g.to_torch(DEV, DEG, raw=raw)
    params = {k: t[k].detach().clone().requires_grad_(True) for k in Trainer.KEYS}
    render_fn = None
    if variant == "b":
        from robosimgs_amd import rasterization

        def render_fn(means, quats, log_scales, logits, colors, *a, **kw):
            return rasterization(means, quats, torch.exp(log_scales), torch.sigmoid(logits), colors, *a, **kw)
    tr = Trainer(params, None, W, H, auto_reorder_every=1_000_000, sh_degree=DEG, render_mode="RGB+ED", isect_capacity=CAP,
                 render_fn=render_fn, raw_params=variant == "c")

    def step():
        for p in params.values():
            p.grad = None
        colors, _, _ = tr.render(vm, K)
        tr.step(l1_loss(colors, target))

    for _ in range(3):                       # warm-up; the first render puts the parameters into Morton order
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
    assert tr.reorders == 1
    return graph, (tr, params, side)


def timed(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="timed replays per variant")
    ap.add_argument("--variant", choices=("a", "b", "c"), default=None, help="replay this variant alone (for a profiler)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = synthetic_scene(N, math.log(0.012), DEG, 0)
    cam = camera_ring(1, W, H, thetas=[0.3])[0]
    vm = torch.from_numpy(cam.viewmat().astype(np.float32)).to(DEV)[None]
    K = torch.from_numpy(cam.K.astype(np.float32)).to(DEV)[None]
    target = torch.rand(1, H, W, 4, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    if a.variant:
        graph, keep = build(a.variant, g, vm, K, target)
        ts = [timed(graph) for _ in range(a.reps)]
        print(json.dumps({"variant": a.variant, "replays": a.reps, "ms_median": round(float(np.median(ts)), 4)}), flush=True)
        return
    graphs, keep = {}, []
    for v in ("a", "b", "c"):
        graphs[v], k = build(v, g, vm, K, target)
        keep.append(k)
    for _ in range(20):                      # warm-up of the replays themselves
        for v in "abc":
            graphs[v].replay()
    torch.cuda.synchronize()
    ts = {v: [] for v in "abc"}
    for _ in range(a.reps):                  # alternated: a b c a b c ...
        for v in "abc":
            ts[v].append(timed(graphs[v]))
    what = {"a": "activated leaves (bench.py's step)", "b": "raw leaves through torch.exp / torch.sigmoid",
            "c": "raw leaves, raw_params=True"}
    med = {}
    for v in "abc":
        x = np.asarray(ts[v])
        med[v] = float(np.median(x))
        print(json.dumps({"variant": v, "what": what[v], "replays": len(x), "ms_median": round(med[v], 4),
                          "ms_min": round(float(x.min()), 4), "ms_p05": round(float(np.percentile(x, 5)), 4),
                          "ms_p95": round(float(np.percentile(x, 95)), 4)}), flush=True)
    xa = np.asarray(ts["a"])
    print(json.dumps({"c_minus_a_ms": round(med["c"] - med["a"], 4), "b_minus_c_ms": round(med["b"] - med["c"], 4),
                      "spread_a_p95_minus_p05_ms": round(float(np.percentile(xa, 95) - np.percentile(xa, 5)), 4)}), flush=True)


if __name__ == "__main__":
    main()
