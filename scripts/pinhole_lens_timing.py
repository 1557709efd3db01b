"""What the pinhole lens costs in the two kernels that evaluate it: project_color_fwd and project_color_bwd at the bench
scene's shape (1 M Gaussians of synthetic_scene, SH degree 3, 1920x1080, the bench's ring camera with its own pinhole K)
under MGS_CAMERA_PINHOLE_BC (the mild lens of the tests) against the plain MGS_CAMERA_PINHOLE.

The protocol is scripts/lens_timing.py's: each variant is a HIP graph of --launches back-to-back launches of the one kernel,
replayed --reps times between two device events, the variants ALTERNATED within the process; the figure is the time per
launch.  Forward in both forms: the training frame (every per-Gaussian output) and the lean inference frame (depths, packed
records and binning seed only).  One JSON line per variant and one with the differences and the spread.

--lib PATH loads another build of libmgs.so (the parent commit's, for its pinhole numbers on the same box); such a library
is timed for the plain pinhole alone.

scripts/pinhole_lens_timing.py [--reps N] [--launches K] [--lib PATH]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"
N, W, H, DEG = 1_000_000, 1920, 1080, 3
MILD = (-0.12, 0.03, 0.002, -0.0015, -0.004)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    from robosimgs_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from robosimgs_amd import camera_ring, ops, synthetic_scene
    torch.cuda.set_device(0)
    g = synthetic_scene(N, math.log(0.012), DEG, 0)
    t = g.to_torch(DEV, DEG)
    cam = camera_ring(1, W, H, thetas=[0.3])[0]
    vm = torch.from_numpy(cam.viewmat().astype(np.float32)).to(DEV)
    K = torch.from_numpy(cam.K.astype(np.float32)).to(DEV)
    cams = {"pinhole": (0, K)}
    have_lens = not a.lib
    if have_lens:
        cams["pinhole_bc"] = (ops.CAMERA_PINHOLE_BC, ops.lens_rows(K[None], None, MILD)[0])

    def fwd(camera, Kc, lean):
        return ops.project_color_fwd_raw(t["means"], t["quats"], t["scales"], t["opacities"], DEG, t["colors"], vm, Kc, W, H,
                                         0.3, 0.01, 1e10, 0.0, False, True, want_splats=True, bin_seed="tight", lean=lean,
                                         camera=camera)
    gen = torch.Generator(DEV).manual_seed(3)
    v_feats = torch.randn(N, 4, device=DEV, generator=gen)
    v_m2d = torch.randn(N, 2, device=DEV, generator=gen)
    v_con = torch.randn(N, 3, device=DEV, generator=gen)
    outs = [torch.empty_like(t[k]) for k in ("means", "quats", "scales", "colors")]

    def bwd(camera, Kc, f):
        ops.project_color_bwd_raw(t["means"], t["quats"], t["scales"], t["opacities"], DEG, t["colors"], vm, Kc, W, H, 0.3,
                                  f[0], f[3], False, f[5], v_feats, v_m2d, v_con, None, *outs, None, camera=camera)
    graphs, info, keep = {}, {}, []           # keep: the forward outputs the backward graphs read
    side = torch.cuda.Stream(DEV)
    for name, (camera, Kc) in cams.items():
        full = fwd(camera, Kc, False)
        keep.append(full)
        info[name] = {"visible": int((full[0] > 0).sum())}
        bodies = {"fwd_train": lambda c=camera, k=Kc: fwd(c, k, False), "fwd_lean": lambda c=camera, k=Kc: fwd(c, k, True),
                  "bwd": lambda c=camera, k=Kc, f=full: bwd(c, k, f)}
        for what, body in bodies.items():
            with torch.cuda.stream(side):
                body()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    for _ in range(a.launches):
                        body()
            torch.cuda.synchronize()
            graphs[(what, name)] = graph

    def timed(graph):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches
    for _ in range(10):
        for graph in graphs.values():
            graph.replay()
    torch.cuda.synchronize()
    ts = {k: [] for k in graphs}
    for _ in range(a.reps):                  # alternated
        for k, graph in graphs.items():
            ts[k].append(timed(graph))
    med = {}
    for (what, name), x in ts.items():
        x = np.asarray(x)
        med[(what, name)] = float(np.median(x))
        print(json.dumps({"kernel": what, "camera": name, "lib": a.lib or "this build", "visible": info[name]["visible"],
                          "replays": len(x), "us_per_launch_median": round(float(np.median(x)), 2),
                          "us_min": round(float(x.min()), 2), "us_p05": round(float(np.percentile(x, 5)), 2),
                          "us_p95": round(float(np.percentile(x, 95)), 2)}), flush=True)
    if have_lens:
        for what in ("fwd_train", "fwd_lean", "bwd"):
            x = np.asarray(ts[(what, "pinhole")])
            print(json.dumps({"kernel": what, "lens_minus_pinhole_us": round(med[(what, "pinhole_bc")] - med[(what, "pinhole")], 2),
                              "pinhole_spread_p95_minus_p05_us": round(float(np.percentile(x, 95) - np.percentile(x, 5)), 2)}),
                  flush=True)


if __name__ == "__main__":
    main()
