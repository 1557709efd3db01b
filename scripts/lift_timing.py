"""Cost of lifting one mask onto the Gaussians (include/mgs_lift.h, csrc/lift.hip) on the BASELINE configs[1] scene: 1 M
Gaussians, 1920x1080, the theta = 0.3 camera, the Gaussians in the caller's order (no Morton reorder).

Per mask -- stripes K = 4, stripes K = 32, checker K = 32 (tests/lift_gates.py's formulas) -- on ONE projection and binning:
  raster_votes_kernel                     the product path
  raster_labels_kernel                    the transpose, K random classes, same lists (what a walk without the reduction costs)
  the backward route                      rasterize_fwd_raw with checkpoints + rasterize_bwd_det_raw at K channels, features
                                          ones [N,K], v_render one-hot(mask): v_feats is the same vote matrix in fp32
and the number of (list entry, present class) pairs per list entry, the upper bound of the atomics issued per pair.
`--resources`: the compiler's resource report of csrc/lift.hip (needs no GPU).

HIP-event times, one process; every variant is warmed up, then timed in `--rounds` windows with the variants taking turns
inside every round; the table gives the median window and the min..max spread.  Needs a GPU: there is no fallback.

    python scripts/lift_timing.py [--rounds 5] [--reps 10] [--out table.md] [--resources]
"""
import argparse
import math
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def resources():
    from robosimgs_amd.csrc import build as B
    src = os.path.join(B.HERE, "lift.hip")
    cmd = [B._hipcc(), *B.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "") for ln in r.stderr.splitlines()
             if "remark:" in ln]
    return [ln.split(":0: ", 1)[-1].strip() for ln in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="launches per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="only print the compiler's resource report")
    a = ap.parse_args()
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(out) + "\n")

    if a.resources:
        for ln in resources():
            say(ln)
        return
    import numpy as np
    import torch
    from robosimgs_amd import camera_ring, ops, synthetic_scene

    dev = torch.device("cuda")
    W, H, n = 1920, 1080, 1_000_000
    t = synthetic_scene(n, math.log(0.012), 0, seed=0).to_torch(dev, 0)
    cam = camera_ring(1, W, H, thetas=[0.3])[0]
    vm = torch.from_numpy(cam.viewmat().astype(np.float32)).to(dev)
    K = torch.from_numpy(cam.K.astype(np.float32)).to(dev)
    tw, th = -(-W // 16), -(-H // 16)
    radii, m2d, dep, con, _ = ops.projection_fwd_raw(t["means"], t["quats"], t["scales"], vm, K, W, H, 0.3, 0.01, 1e10, 0.0, False)
    opac = t["opacities"]
    probe = ops.isect_tiles_raw(m2d, radii, dep, tw, th, 24_000_000, conics=con, opacities=opac)
    n_isect = int(probe.n_isect.item())
    assert int(probe.status.item()) == 0
    del probe
    tl = ops.isect_tiles_raw(m2d, radii, dep, tw, th, n_isect + 1, conics=con, opacities=opac, want_pair_info=True)
    assert int(tl.status.item()) == 0 and int(tl.n_isect.item()) == n_isect
    lens = (tl.tile_offsets[1:] - tl.tile_offsets[:-1]).view(th, tw)
    say(f"configs[1]: {n} Gaussians, {W}x{H}, {n_isect} tile intersections, {tw * th} tiles, caller's order")

    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    masks = {"stripes K = 4": ((xx * 4 // W).to(torch.uint8), 4),
             "stripes K = 32": ((xx * 32 // W).to(torch.uint8), 32),
             "checker K = 32": ((((xx // 4) + 5 * (yy // 4)) % 32).to(torch.uint8), 32)}
    rng = np.random.default_rng(5)
    lab = (torch.empty(H, W, dtype=torch.uint8, device=dev), torch.empty(H, W, device=dev))
    segment = 256
    rows = []
    for name, (mask, k) in masks.items():
        # (list entry, present class) pairs per list entry: what the reduction loop runs, the upper bound of the atomics
        padded = torch.full((th * 16, tw * 16), 255, dtype=torch.uint8, device=dev)
        padded[:H, :W] = mask
        present = torch.stack([(padded == c).view(th, 16, tw, 16).any(dim=3).any(dim=1) for c in range(k)]).sum(dim=0)
        per_pair = float((present * lens).sum()) / n_isect
        votes = torch.zeros(n, k, dtype=torch.int64, device=dev)
        cls = torch.from_numpy(rng.integers(0, k, n).astype(np.int32)).to(dev)
        feats = torch.ones(n, k, device=dev)
        v_render = torch.nn.functional.one_hot(mask.long(), k).float().contiguous()
        ckpt = ops.checkpoint_buffer(n_isect + 1, tw, th, k, segment, dev)
        frame = (torch.empty(H, W, k, device=dev), torch.empty(H, W, device=dev), torch.empty(H, W, dtype=torch.int32, device=dev))

        def lift():
            ops.raster_votes_raw(tl, mask, k, W, H, votes, means2d=m2d, conics=con, opacities=opac)

        def labels():
            ops.raster_labels_raw(tl, cls, k, W, H, means2d=m2d, conics=con, opacities=opac, out=lab)

        def backward_route():
            ops.rasterize_fwd_raw(m2d, con, feats, opac, None, W, H, tw, th, tl.tile_offsets, tl.flatten_ids, out=frame,
                                  group_order=tl.group_order, checkpoints=ckpt, checkpoint_interval=segment)
            return ops.rasterize_bwd_det_raw(m2d, con, feats, opac, None, W, H, tw, th, tl, frame[1], frame[2], v_render, None,
                                             render_out=frame[0], checkpoints=ckpt, checkpoint_interval=segment)[2]

        # the two routes give the same matrix: shown once per mask before anything is timed
        votes.zero_()
        lift()
        v_feats = backward_route()
        diff = float((ops.votes_to_float(votes) - v_feats.double()).abs().max())
        scale = float(v_feats.abs().max())
        variants = {"raster_votes_kernel": lift, "raster_labels_kernel": labels, "backward route": backward_route}
        times = {v: [] for v in variants}
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for v, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        med = {v: statistics.median(x) for v, x in times.items()}
        rows.append((name, med, {v: (min(x), max(x)) for v, x in times.items()}, per_pair, diff, scale))
        say(f"{name}: votes {med['raster_votes_kernel']:.1f} us, labels {med['raster_labels_kernel']:.1f} us, backward route "
            f"{med['backward route']:.1f} us; {per_pair:.2f} reductions per list entry; largest difference between the two "
            f"vote matrices {diff:.2e} at a largest vote of {scale:.1f}")
        del votes, feats, v_render, ckpt, frame, v_feats
        torch.cuda.empty_cache()
    say()
    say("| mask | raster_votes_kernel us (min .. max) | raster_labels_kernel us | backward route us (min .. max) | backward / votes "
        "| reductions per list entry |")
    say("|---|---|---|---|---|---|")
    for name, med, span, per_pair, _, _ in rows:
        v, l, b = med["raster_votes_kernel"], med["raster_labels_kernel"], med["backward route"]
        say(f"| {name} | {v:.1f} ({span['raster_votes_kernel'][0]:.1f} .. {span['raster_votes_kernel'][1]:.1f}) | {l:.1f} | "
            f"{b:.1f} ({span['backward route'][0]:.1f} .. {span['backward route'][1]:.1f}) | {b / v:.2f} | {per_pair:.2f} |")


if __name__ == "__main__":
    main()
