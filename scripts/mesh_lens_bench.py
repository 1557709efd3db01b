"""Measure the mesh rasteriser under a lens on the GPU, beside the plain pinhole path in the same process
(profiles/mesh_lens/README.md).  The companion of scripts/mesh_bench.py:

    python scripts/mesh_lens_bench.py                    # whole renders and the lens stages, device events
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/mesh_lens_bench.py --profile
    python scripts/mesh_lens_bench.py --parse DIR        # per-kernel median and spread from that trace

Two configurations of the open box (25,000 faces) seen from the pin's `top` camera, under the mild pinhole lens of
tests/pinhole_lens_ref.py (its coefficients are in normalised units, so the view's own K carries them to the frame):
1920 x 1080 (510 superblocks in a face's box scan) and 3840 x 2160 (2,040).  In each, PROFILE_CALLS renders of the pinhole
path and then as many of the lens path."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import mesh_scenes as MS          # noqa: E402
import pinhole_lens_ref as PR     # noqa: E402
from mesh_bench import KERNELS as PINHOLE, kernel_of, stats      # noqa: E402

# the same text as the pinhole's rows (csrc/mesh_kernels.h), instantiated for LensView
LENS = ["mesh_vertices_kernel", "mesh_rays_kernel", "mesh_lens_blocks_kernel", "mesh_lens_supers_kernel", "mesh_clear_kernel",
        "mesh_faces_kernel<LensView>", "mesh_large_kernel<LensView>", "mesh_resolve_kernel<LensView>"]
PROFILE_CALLS = 40
WARM = 10


def configs():
    box = MS.openbox()
    vm, K = MS.top_1080p(box)
    return box, {"top_1080p": (vm, K, 1920, 1080), "top_2160p": (vm, MS.scaled_K(K, 2.0), 3840, 2160)}


def parse(directory):
    """Per configuration, path and kernel: median / p10 / p90 of the dispatch durations in a trace of --profile."""
    # mesh_vertices_kernel and mesh_clear_kernel carry the same name on both paths: their rows are told apart by their place
    # in the dispatch sequence (PROFILE_CALLS pinhole renders, then as many under the lens), which the assert below holds
    names = sorted(set(PINHOLE + LENS))
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            for r in csv.DictReader(fh):
                name = kernel_of(r["Kernel_Name"], names)
                if name:
                    rows.append((int(r["Start_Timestamp"]), name, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    at = 0
    for cfg in ("top_1080p", "top_2160p"):
        for path, kernels in (("pinhole", PINHOLE), ("lens", LENS)):
            n = len(kernels) * PROFILE_CALLS
            chunk = rows[at + len(kernels) * WARM:at + n]
            at += n
            assert [k for _, k, _ in chunk[:len(kernels)]] == kernels, (cfg, path, [k for _, k, _ in chunk[:len(kernels)]])
            out = {k: stats([d * 1e-6 for _, nm, d in chunk if nm == k]) for k in kernels}
            out["sum_of_medians_us"] = round(sum(out[k]["median_us"] for k in kernels), 2)
            print(json.dumps({"config": cfg, "path": path, "kernels": out}))
    assert at == len(rows), f"{len(rows)} mesh dispatches in the trace, {at} expected"


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
    from robosimgs_amd import Mesh, MeshRenderer, mesh_lens_rays, mesh_raster, mesh_resolve
    assert torch.cuda.is_available(), "mesh_lens_bench measures on the GPU; there is no other path"
    box, cfgs = configs()
    dev = "cuda"
    mesh = Mesh(box["verts"], box["faces"]).to(dev)
    for name, (vm, K, W, H) in cfgs.items():
        plain = MeshRenderer(mesh, W, H, headlight=True)
        lens = MeshRenderer(mesh, W, H, headlight=True, pinhole_distortion=PR.MILD)
        vmd, Kd = torch.from_numpy(vm[None].copy()).to(dev), torch.from_numpy(K[None].copy()).to(dev)
        if args.profile:
            for r in (plain, lens):
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

        res = {"config": name, "lib": args.lib or "libmgs.so", "render_pinhole": timed(lambda: plain.render(vmd, Kd)), "render_lens": timed(lambda: lens.render(vmd, Kd))}
        _, _, meta = lens.render(vmd, Kd)
        m = mesh_lens_rays(Kd, W, H, pinhole_distortion=PR.MILD)
        res["stage_rays"] = timed(lambda: mesh_lens_rays(Kd, W, H, pinhole_distortion=PR.MILD, workspace=m.workspace))
        vc = lens.verts_cam
        res["stage_raster_lens"] = timed(lambda: mesh_raster(vc, mesh.faces, Kd, W, H, workspace=lens.workspace, rays=m))
        res["stage_resolve_lens"] = timed(lambda: mesh_resolve(vc, mesh.faces, Kd, W, H, lens.workspace, headlight=True, out=lens.out, rays=m))
        res["stage_raster_pinhole"] = timed(lambda: mesh_raster(vc, mesh.faces, Kd, W, H, workspace=plain.workspace))
        res["covered_px_pinhole"] = int((plain.out["face_ids"] >= 0).sum())
        res["covered_px_lens"] = int((meta["face_ids"] >= 0).sum())
        res["pixels_without_a_ray"] = int(torch.isnan(meta["rays"]).any(-1).sum())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
