"""Measure the mesh rasteriser on the GPU, in a process that holds nothing but the mesh renderer (profiles/mesh/README.md).

    python scripts/mesh_bench.py                         # whole render and the stage entry points, device events
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/mesh_bench.py --profile
    python scripts/mesh_bench.py --parse DIR             # per-kernel median and spread from that trace

Three configurations of the open box (25,000 faces): `top` at 800 x 800, `top` at 1920 x 1080, and the 1920 x 1080 close-up
with more than a thousand faces on the large-face path.  Every time is a median over --calls calls after --warmup, with the
10th and 90th percentile; beside it the byte floor of the contract bytes at 8 TB/s: clear 8 B/px written, resolve 8 B/px
read + 20 B/px written, vertices 12 B read + 12 B written each, the visibility updates 8 B each (their count: the keys the
host harness forms for the same scene, i.e. the atomics of a kernel without the plain-load test)."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_scenes as MS          # noqa: E402

PEAK = 8e12                       # bytes / s, the figure the project's other rooflines use
# the raster and resolve kernels are one text per view (csrc/mesh_kernels.h): the pinhole's rows are the PinholeViews ones
KERNELS = ["mesh_vertices_kernel", "mesh_clear_kernel", "mesh_faces_kernel<PinholeViews>", "mesh_large_kernel<PinholeViews>",
           "mesh_resolve_kernel<PinholeViews>"]
PROFILE_CALLS = 40


def configs():
    box = MS.openbox()
    v = box["views"]["top"]
    return box, {"top_800": (v["viewmat"], v["K"], 800, 800), "top_1080p": (*MS.top_1080p(box), 1920, 1080),
                 "closeup_1080p": (*MS.closeup_1080p(box), 1920, 1080)}


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_us": round(float(np.median(a)) * 1e3, 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]) * 1e3, 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]) * 1e3, 2), "n": len(a)}


def floors(box, W, H, keys):
    V = len(box["verts"])
    b = {"clear": 8 * W * H, "vertices": 24 * V, "faces": 8 * int(keys), "resolve": 28 * W * H}
    return {k: {"bytes": v, "floor_us": round(v / PEAK * 1e6, 3)} for k, v in b.items()}


def kernel_of(row_name, kernels):
    """The entry of `kernels` a profiler row names, or None: `name` for a plain kernel, `name<View>` for an instantiation (the
    row carries the view's qualified name as the template argument, or its mangled form).  No kernel's name contains another's."""
    for k in kernels:
        base, _, view = k.partition("<")
        if base in row_name and view.rstrip(">") in row_name:
            return k
    return None


def parse(directory):
    """Per configuration and kernel: median / p10 / p90 of the dispatch durations in a rocprofv3 kernel trace of --profile."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            for r in csv.DictReader(fh):
                name = kernel_of(r["Kernel_Name"], KERNELS)
                if name:
                    rows.append((int(r["Start_Timestamp"]), name, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    per = 5 * PROFILE_CALLS
    assert len(rows) == 3 * per, f"{len(rows)} mesh dispatches in the trace, {3 * per} expected"
    for i, name in enumerate(("top_800", "top_1080p", "closeup_1080p")):
        chunk = rows[i * per + 5 * 10:(i + 1) * per]                 # the first ten calls of a configuration are warm-up
        out = {k: stats([d * 1e-6 for _, n, d in chunk if n == k]) for k in KERNELS}
        out["sum_of_medians_us"] = round(sum(out[k]["median_us"] for k in KERNELS), 2)
        print(json.dumps({"config": name, "kernels": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lib", default=None, help="another build of libmgs.so to measure (an A/B of one kernel)")
    ap.add_argument("--profile", action="store_true", help="only enqueue renders, for a rocprofv3 kernel trace")
    ap.add_argument("--parse", default=None)
    args = ap.parse_args()
    if args.parse:
        return parse(args.parse)
    import torch
    from robosimgs_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from robosimgs_amd import Mesh, MeshRenderer, mesh_raster, mesh_resolve, mesh_vertices
    assert torch.cuda.is_available(), "mesh_bench measures on the GPU; there is no other path"
    box, cfgs = configs()
    dev = "cuda"
    mesh = Mesh(box["verts"], box["faces"]).to(dev)
    harness = None if args.profile else MS.build_harness(os.environ.get("TMPDIR", "/tmp"))
    for name, (vm, K, W, H) in cfgs.items():
        r = MeshRenderer(mesh, W, H, headlight=True)
        vmd, Kd = torch.from_numpy(vm[None].copy()).to(dev), torch.from_numpy(K[None].copy()).to(dev)
        if args.profile:
            for _ in range(PROFILE_CALLS):
                r.render(vmd, Kd)
            torch.cuda.synchronize()
            continue

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            return stats([a.elapsed_time(b) for a, b in ev])

        res = {"config": name, "lib": args.lib or "libmgs.so", "render_eager": timed(lambda: r.render(vmd, Kd))}
        g = torch.cuda.CUDAGraph()                                   # the renderer alone, one linear graph
        with torch.cuda.graph(g):
            r.render(vmd, Kd)
        res["render_graph_replay"] = timed(g.replay)
        vc = torch.empty_like(r.verts_cam)
        res["stage_vertices"] = timed(lambda: mesh_vertices(mesh.vertices, vmd, out=vc))
        res["stage_raster"] = timed(lambda: mesh_raster(vc, mesh.faces, Kd, W, H, workspace=r.workspace))
        res["stage_resolve"] = timed(lambda: mesh_resolve(vc, mesh.faces, Kd, W, H, r.workspace, headlight=True, out=r.out))
        ids = r.out["face_ids"]
        o = MS.harness_render(harness, box["verts"], box["faces"], vm[None], K[None], W, H, headlight=True)
        res["covered_px"], res["keys"], res["large_faces"] = int((ids >= 0).sum()), int(o["keys"][0]), int(o["listed"][0])
        res["same_ids_as_host_harness"] = bool(np.array_equal(ids[0].cpu().numpy(), o["face_ids"][0]))
        res["floors"] = floors(box, W, H, res["keys"])
        res["floor_total_us"] = round(sum(v["floor_us"] for v in res["floors"].values()), 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
