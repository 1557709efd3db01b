"""Cost of the part-label output (include/mgs_labels.h, csrc/labels.hip) on the BASELINE configs[1] scene: 1 M Gaussians,
SH degree 3, 1920x1080, the theta = 0.3 camera.

(i)   raster_labels_kernel alone for K = 2, 8 and 32 random classes against raster_fwd_kernel alone (inference variant,
      throughput schedule, RGB + expected depth) on the same packed records and the same lists;
(ii)  FrameRenderer frames/s with three frames in flight, label frames on (K = 8) against off;
(iii) the compiler's resource report of the kernel (`--resources`: hipcc -Rpass-analysis=kernel-resource-usage on
      csrc/labels.hip with the library's flags; needs no GPU).

HIP-event times (i) and wall-clock rates over whole windows (ii), one process.  Every variant is warmed up, then timed in
`--rounds` windows with the variants taking turns inside every round, so that drift and neighbours hit all of them alike;
the tables give the median window and the min..max spread.  Needs a GPU for (i) and (ii): there is no fallback.

    python scripts/labels_timing.py [--rounds 7] [--reps 20] [--frames 300] [--out table.md] [--resources]
"""
import argparse
import math
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def resources():
    from robosimgs_amd.csrc import build as B
    src = os.path.join(B.HERE, "labels.hip")
    cmd = [B._hipcc(), *B.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "") for ln in r.stderr.splitlines()
             if "remark:" in ln]
    return [ln.split(":0: ", 1)[-1].strip() for ln in lines]      # (drop the file:line:column prefix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="launches per timed window of (i)")
    ap.add_argument("--frames", type=int, default=300, help="frames per timed window of (ii)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="only print the compiler's resource report")
    a = ap.parse_args()
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    if a.resources:
        for ln in resources():
            say(ln)
        return
    import numpy as np
    import torch
    from robosimgs_amd import FrameRenderer, camera_ring, ops, synthetic_scene

    dev = torch.device("cuda")
    W, H, deg, n = 1920, 1080, 3, 1_000_000
    t = synthetic_scene(n, math.log(0.012), deg, seed=0).to_torch(dev, deg)
    cam = camera_ring(1, W, H, thetas=[0.3])[0]
    vm = torch.from_numpy(cam.viewmat().astype(np.float32)).to(dev)
    K = torch.from_numpy(cam.K.astype(np.float32)).to(dev)
    tw, th = -(-W // 16), -(-H // 16)

    # ---- (i) the two kernels alone, on one projection and one binning ----------------------------------------------------
    _, _, depths, _, _, _, splats, seed = ops.project_color_fwd_raw(
        t["means"], t["quats"], t["scales"], t["opacities"], deg, t["colors"], vm, K, W, H, 0.3, 0.01, 1e10, 0.0, False, True,
        want_splats=True, bin_seed="tight", lean=True)
    tl = ops.isect_tiles_raw(None, None, depths, tw, th, 24_000_000, seed=seed, want_tile_ids=False, want_tiles_per_gauss=False)
    n_isect = int(tl.n_isect.item())
    assert int(tl.status.item()) == 0
    say(f"configs[1]: {n} Gaussians, SH {deg}, {W}x{H}, {n_isect} tile intersections, {tw * th} tiles")
    frame = (torch.empty(H, W, 4, device=dev), torch.empty(H, W, device=dev), None)
    rng = np.random.default_rng(5)
    classes = {k: torch.from_numpy(rng.integers(0, k, n).astype(np.int32)).to(dev) for k in (2, 8, 32)}
    lab = (torch.empty(H, W, dtype=torch.uint8, device=dev), torch.empty(H, W, device=dev))

    def fwd():
        ops.rasterize_fwd_raw(None, None, None, None, None, W, H, tw, th, tl.tile_offsets, tl.flatten_ids, out=frame,
                              track_last=False, splats=splats, expected_last=True, latency=False, group_order=tl.group_order,
                              channels=4)

    variants = {"raster_fwd_kernel (throughput schedule, 4 channels)": fwd}
    for k, cls in classes.items():
        variants[f"raster_labels_kernel K = {k}"] = (lambda k=k, cls=cls: ops.raster_labels_raw(tl, cls, k, W, H, splats=splats, out=lab))
    times = {name: [] for name in variants}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    say()
    say("| kernel alone, same records and lists | us per launch (median of windows) | min .. max | vs forward |")
    say("|---|---|---|---|")
    base = statistics.median(times[next(iter(times))])
    for name, v in times.items():
        say(f"| {name} | {statistics.median(v):.1f} | {min(v):.1f} .. {max(v):.1f} | {statistics.median(v) / base:.2f} |")

    # ---- (ii) frames in flight ---------------------------------------------------------------------------------------------
    cam_dev = FrameRenderer.pack_camera(vm, K)
    kw = dict(render_mode="RGB+ED", frames_in_flight=3, sizing_camera=(cam.viewmat(), cam.K), capacity_margin=1.25)
    renderers = {"labels off": FrameRenderer(t, W, H, **kw),
                 "labels on (K = 8)": FrameRenderer(t, W, H, class_ids=classes[8], n_classes=8, **kw)}

    def fps(fr, frames):
        tickets = []

        def push():
            if len(tickets) == fr.n_slots:
                tk = tickets.pop(0)
                fr.fetch(tk, check=False)
                fr.release(tk)
            tickets.append(fr.submit(cam_dev))
        for _ in range(6):
            push()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            push()
        while tickets:
            tk = tickets.pop(0)
            fr.fetch(tk, check=False)
            fr.release(tk)
        torch.cuda.synchronize()
        return frames / (time.perf_counter() - t0)

    rates = {name: [] for name in renderers}
    for rnd in range(a.rounds):
        for name, fr in renderers.items():
            rates[name].append(fps(fr, a.frames))
    assert all(fr.isect_status_max() == 0 for fr in renderers.values())
    say()
    say("| FrameRenderer, three frames in flight | frames/s (median of windows, the first dropped) | min .. max |")
    say("|---|---|---|")
    for name, v in rates.items():
        v = v[1:] if len(v) > 1 else v
        say(f"| {name} | {statistics.median(v):.0f} | {min(v):.0f} .. {max(v):.0f} |")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
