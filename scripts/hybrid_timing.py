"""Cost of the exact mesh-over-splat composite (include/mgs_hybrid.h, csrc/hybrid.hip) on the BASELINE configs[1] scene:
1 M Gaussians, SH degree 3, 1920x1080, the theta = 0.3 camera, with the reference's open box (tests/golden) rendered by
MeshRenderer from the same camera as the foreground.

(i)   raster_over_opaque_kernel alone (and with an empty foreground: the copy of the frame alone), beside composite_over
      and raster_fwd_kernel (inference variant, throughput schedule: one wave per tile, RGB + expected depth) alone, all
      on one projection, one binning and one frame;
(ii)  what the kernel walks: the share of tiles with an open pixel, and the mean truncated list length of those tiles
      against their full one, from the offsets and depths -- and with them the estimate
      (list entries walked / list entries of the frame) x the forward's time, to set beside the kernel's time;
(iii) the compiler's resource report of the kernel (`--resources`: hipcc -Rpass-analysis=kernel-resource-usage on
      csrc/hybrid.hip with the library's flags; needs no GPU).

HIP-event times, one process.  Every variant is warmed up, then timed in `--rounds` windows with the variants taking
turns inside every round; the table gives the median window and the min..max spread.  Needs a GPU for (i) and (ii).

    python scripts/hybrid_timing.py [--rounds 7] [--reps 20] [--out table.md] [--resources]
"""
import argparse
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resources():
    from robosimgs_amd.csrc import build as B
    src = os.path.join(B.HERE, "hybrid.hip")
    cmd = [B._hipcc(), *B.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "") for ln in r.stderr.splitlines()
             if "remark:" in ln]
    return [ln.split(":0: ", 1)[-1].strip() for ln in lines]      # (drop the file:line:column prefix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="launches per timed window")
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
    from robosimgs_amd import Mesh, MeshRenderer, camera_ring, composite_over, ops, synthetic_scene

    dev = torch.device("cuda")
    W, H, deg, n = 1920, 1080, 3, 1_000_000
    t = synthetic_scene(n, math.log(0.012), deg, seed=0).to_torch(dev, deg)
    cam = camera_ring(1, W, H, thetas=[0.3])[0]
    vm = torch.from_numpy(cam.viewmat().astype(np.float32)).to(dev)
    K = torch.from_numpy(cam.K.astype(np.float32)).to(dev)
    tw, th = -(-W // 16), -(-H // 16)

    # one projection (arrays and packed records), one binning, one frame
    radii, m2d, depths, con, _, feats, splats, seed = ops.project_color_fwd_raw(
        t["means"], t["quats"], t["scales"], t["opacities"], deg, t["colors"], vm, K, W, H, 0.3, 0.01, 1e10, 0.0, False, True,
        want_splats=True, bin_seed="tight")
    opac = t["opacities"]
    tl = ops.isect_tiles_raw(None, None, depths, tw, th, 24_000_000, seed=seed, want_tile_ids=False, want_tiles_per_gauss=False)
    n_isect = int(tl.n_isect.item())
    assert int(tl.status.item()) == 0
    say(f"configs[1]: {n} Gaussians, SH {deg}, {W}x{H}, {n_isect} tile intersections, {tw * th} tiles")
    frame = (torch.empty(H, W, 4, device=dev), torch.empty(H, W, device=dev), None)

    def fwd(records=True):
        ops.rasterize_fwd_raw(None if records else m2d, None if records else con, None if records else feats,
                              None if records else opac, None, W, H, tw, th, tl.tile_offsets, tl.flatten_ids, out=frame,
                              track_last=False, splats=splats if records else None, expected_last=True, latency=False,
                              group_order=tl.group_order, channels=4)

    fwd()
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_openbox.npz"))
    verts = np.concatenate([g["lid_vertices"], g["body_vertices"]]).astype(np.float32)
    faces = np.concatenate([g["lid_faces"].astype(np.int64), g["body_faces"].astype(np.int64) + len(g["lid_vertices"])])
    mesh = MeshRenderer(Mesh(verts, faces).to(dev), W, H, headlight=True)
    fg_rgb, fg_depth, _ = mesh.render(vm[None], K[None])
    fg_rgb, fg_depth = fg_rgb[0].contiguous(), fg_depth[0].contiguous()
    hyb = (torch.empty(H, W, 3, device=dev), torch.empty(H, W, device=dev), torch.empty(H, W, device=dev))
    bd = torch.tensor([0.05, 0.05, 0.08], device=dev)

    # ---- (ii) what the kernel walks ------------------------------------------------------------------------------------------
    z = depths.cpu().numpy()
    ids = tl.flatten_ids[:n_isect].cpu().numpy()
    offs = tl.tile_offsets.cpu().numpy().astype(np.int64)
    d = fg_depth.cpu().numpy()
    has = (d > 0) & (d < np.inf)
    full, trunc, walked = np.diff(offs), np.zeros(tw * th, np.int64), np.zeros(tw * th, bool)
    for tile in range(tw * th):
        ty, tx = divmod(tile, tw)
        sl = (slice(ty * 16, min(ty * 16 + 16, H)), slice(tx * 16, min(tx * 16 + 16, W)))
        if has[sl].any():
            walked[tile] = True
            trunc[tile] = np.searchsorted(z[ids[offs[tile]:offs[tile + 1]]], d[sl][has[sl]].max(), side="left")
    share = walked.mean()
    work = trunc.sum() / max(1, full.sum())
    say(f"foreground: {int(has.sum())} pixels ({has.mean():.2%} of the frame); tiles with an open pixel: {int(walked.sum())} of "
        f"{tw * th} ({share:.2%})")
    say(f"those tiles: mean full list {full[walked].mean():.0f} entries, mean truncated list {trunc[walked].mean():.0f} "
        f"({trunc[walked].sum() / max(1, full[walked].sum()):.2%}); all tiles: mean full list {full.mean():.0f}")
    say(f"list entries walked / list entries of the frame: {work:.4f}; longest truncated list {int(trunc.max())} entries "
        f"(longest full list of the frame {int(full.max())})")

    # ---- (i) the kernels alone ------------------------------------------------------------------------------------------------
    def hybrid():
        ops.raster_over_opaque_raw(tl, m2d, con, opac, feats, depths, fg_rgb, fg_depth, frame[0], frame[1], W, H, backdrop=bd,
                                   out=hyb)

    def composite():
        composite_over(frame[0][..., :3], frame[1], frame[0][..., 3], fg_rgb, fg_depth, backdrop=(0.05, 0.05, 0.08))

    no_fg = torch.zeros_like(fg_depth)

    def pass_through():
        ops.raster_over_opaque_raw(tl, m2d, con, opac, feats, depths, fg_rgb, no_fg, frame[0], frame[1], W, H, backdrop=bd, out=hyb)

    variants = {"raster_fwd_kernel (throughput schedule, 4 channels, packed records)": fwd,
                "raster_fwd_kernel (the same, from means2d / conics / feats / opacities)": lambda: fwd(False),
                "composite_over (with its wrapper's copies and allocations)": composite,
                "raster_over_opaque_kernel": hybrid,
                "raster_over_opaque_kernel, no foreground anywhere (every tile copies the frame)": pass_through}
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
    say("| alone, same projection, lists and frame | us per call (median of windows) | min .. max |")
    say("|---|---|---|")
    for name, v in times.items():
        say(f"| {name} | {statistics.median(v):.1f} | {min(v):.1f} .. {max(v):.1f} |")
    med = {name: statistics.median(v) for name, v in times.items()}
    names = list(variants)
    est = work * med[names[1]]
    say()
    say(f"estimate (entries walked / entries of the frame) x forward from arrays = {work:.4f} x {med[names[1]]:.1f} us = "
        f"{est:.1f} us; measured {med[names[3]]:.1f} us; measured / estimate = {med[names[3]] / max(est, 1e-9):.2f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
