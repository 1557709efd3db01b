"""What fusing and meshing cost (robosimgs_amd/tsdf.py): HIP-event times of TSDFVolume.integrate for C = 1, 8 and 32 views of
1920 x 1080 and of the two extraction calls, at 256^3 and 512^3 samples with colour, on bench.py's 1 M-Gaussian scene seen from
its camera ring; next to them the time the volume's own traffic would take at the HBM rate measured here with a device copy
of the same size (the floor of one pass: every sample's 20 bytes read and written once).

The frames are rendered once, before anything is timed.  integrate is timed as called from Python on a volume that already
holds the views (steady state: every sample a view sees is read, updated and written); every case is warmed up, the cases
are taken in alternating rounds.  The extraction is timed per entry point through the raw layer (counts already known, so no
read-back sits between the events) and once more as extract_arrays with its read-back, by a host clock.
Prints one JSON line per case.   scripts/bench_tsdf.py [--n N --reps R --rounds K --sizes 256 512 --views 1 8 32]"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from robosimgs_amd import TSDFVolume, camera_ring, rasterization, synthetic_scene  # noqa: E402
from robosimgs_amd import _lib  # noqa: E402
from robosimgs_amd._lib import check, ptr, stream_handle  # noqa: E402

DEV = "cuda"


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


def measure(fns, reps, rounds, warmup=3):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k] += event_times(fn, reps)
    return out


def render_views(n, views, width, height, extent):
    scene = synthetic_scene(n, math.log(0.012), 3, seed=0, extent=extent).to_torch(DEV)
    cams = camera_ring(views, width, height)
    vm = torch.from_numpy(np.stack([c.viewmat() for c in cams]).astype(np.float32)).to(DEV)
    Ks = torch.from_numpy(np.stack([c.K for c in cams]).astype(np.float32)).to(DEV)
    frames = torch.empty(views, height, width, 4, device=DEV)
    alphas = torch.empty(views, height, width, 1, device=DEV)
    for i in range(views):                                   # one view at a time: the renderer's buffers stay one frame large
        c, a, _ = rasterization(scene["means"], scene["quats"], scene["scales"], scene["opacities"], scene["colors"],
                                vm[i:i + 1], Ks[i:i + 1], width, height, sh_degree=3, render_mode="RGB+ED")
        frames[i], alphas[i] = c[0], a[0]
    del scene
    return frames, alphas, vm, Ks


def extract_calls(vol):
    """The two entry points as closures on buffers sized once (the raw layer's calls, without its read-back)."""
    L, v, stream = _lib.lib(), vol._struct(), stream_handle()
    nbytes = ctypes.c_size_t(0)
    check(L.mgs_tsdf_extract_count(ctypes.byref(v), 0.0, 1.0, None, None, ctypes.byref(nbytes), stream), "size query")
    ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr() % 256)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    count = lambda: check(L.mgs_tsdf_extract_count(ctypes.byref(v), 0.0, 1.0, ptr(counts), base, ctypes.byref(nbytes), stream),
                          "mgs_tsdf_extract_count")
    count()
    n_v, n_f = (int(x) for x in counts.tolist())
    vertices = torch.empty(max(n_v, 1), 3, device=DEV)
    colors = torch.empty(max(n_v, 1), 3, device=DEV)
    faces = torch.empty(max(n_f, 1), 3, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    emit = lambda: check(L.mgs_tsdf_extract_emit(ctypes.byref(v), 0.0, 1.0, ptr(counts), base, nbytes.value, ptr(vertices),
                                                 ptr(colors), n_v, ptr(faces), n_f, ptr(status), stream), "mgs_tsdf_extract_emit")
    return count, emit, n_v, n_f, nbytes.value


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--extent", type=float, default=3.0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    frames, alphas, vm, Ks = render_views(a.n, max(a.views), a.width, a.height, a.extent)
    torch.cuda.synchronize()
    stat = lambda ts: dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4))
    for size in a.sizes:
        vol = TSDFVolume.from_bounds((-a.extent,) * 3, (a.extent,) * 3, 2 * a.extent / size, device=DEV)
        samples = size ** 3
        vol.integrate(frames, vm, Ks, alphas=alphas)             # the state every timed call starts from
        seen = float((vol.weight > 0).float().mean())
        # the floor: 20 bytes of every sample read and written once, at the rate a device copy of that size reaches here
        src = torch.empty(samples * 5, device=DEV)
        dst = torch.empty_like(src)
        copy = measure({"copy": lambda: dst.copy_(src)}, a.reps, a.rounds)["copy"]
        rate = 2 * src.numel() * 4 / (float(np.median(copy)) * 1e-3)
        del src, dst
        floor_ms = 2 * 20 * samples / rate * 1e3
        print(json.dumps({"case": "device copy", "size": size, "bytes_moved": 2 * 20 * samples, "GB_per_s": round(rate / 1e9, 1),
                          "volume_pass_floor_ms": round(floor_ms, 4), **stat(copy)}), flush=True)
        fns = {f"integrate C={c}": (lambda c=c: vol.integrate(frames[:c], vm[:c], Ks[:c], alphas=alphas[:c])) for c in a.views}
        for k, ts in measure(fns, a.reps, a.rounds).items():
            print(json.dumps({"case": k, "size": size, "frame": [a.height, a.width], "samples_seen_share": round(seen, 3),
                              "over_floor": round(float(np.median(ts)) / floor_ms, 2), **stat(ts)}), flush=True)
        # the frame layout alone: a volume without colour fed the 16-byte RGB+ED pixels, then a packed [C,H,W] depth plane with
        # the alpha test folded in (the same updates, the same 8 bytes per sample of volume traffic)
        c = a.views[len(a.views) // 2]
        plain = TSDFVolume.from_bounds((-a.extent,) * 3, (a.extent,) * 3, 2 * a.extent / size, color=False, device=DEV)
        packed = torch.where(alphas[:c, ..., 0] >= 0.5, frames[:c, ..., 3], torch.zeros((), device=DEV)).contiguous()
        plain.integrate(frames, vm, Ks, alphas=alphas)
        fns = {f"integrate C={c}, no colour, RGB+ED frame": lambda: plain.integrate(frames[:c], vm[:c], Ks[:c], alphas=alphas[:c]),
               f"integrate C={c}, no colour, packed depth": lambda: plain.integrate(packed, vm[:c], Ks[:c])}
        for k, ts in measure(fns, a.reps, a.rounds).items():
            print(json.dumps({"case": k, "size": size, **stat(ts)}), flush=True)
        del plain, packed
        count, emit, n_v, n_f, ws_bytes = extract_calls(vol)
        for k, ts in measure({"extract_count": count, "extract_emit": emit}, a.reps, a.rounds).items():
            print(json.dumps({"case": k, "size": size, "vertices": n_v, "faces": n_f, "workspace_bytes": ws_bytes, **stat(ts)}),
                  flush=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, f, c = vol.extract_arrays()
        torch.cuda.synchronize()
        print(json.dumps({"case": "extract_arrays (host clock, with its read-back and allocations)", "size": size,
                          "ms": round((time.perf_counter() - t0) * 1e3, 3), "vertices": v.shape[0], "faces": f.shape[0]}), flush=True)
        del vol, v, f, c
