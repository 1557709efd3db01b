"""Timing of the pose backward (mgs_pose_bwd, csrc/pose.hip) in the shape of scripts/transform_timing.py: 1 M Gaussians,
8 groups, SH degree 3, device events, warm-up, 50 calls.  Three cases -- all moving with SH, all moving without SH, 10 %
moving -- and for each: the backward call alone, forward plus backward through pose_gaussians, and, alternating with
them in the same run, the same gradients composed from torch ops (`torch_backward` below: the only baseline there is).
Beside each time of the backward: the bytes the algorithm needs, from the shapes, and their share of 8 TB/s.

    python scripts/pose_timing.py [--blocks]      # --blocks: group ids part by part (contiguous) instead of random
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robosimgs_amd import synthetic_scene  # noqa: E402
from robosimgs_amd.pose import (pack_transforms_torch, pose_bwd_raw, pose_gaussians, sh_generator_matrices,  # noqa: E402
                                workspace_bytes)
from robosimgs_amd.transform import transform_gaussians  # noqa: E402

N, G, DEG, CALLS, WARMUP, PEAK = 1_000_000, 8, 3, 50, 3, 8e12


def quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def torch_backward(posed, cts, gid, xd, rd, gens, sh):
    """mgs_pose_bwd's results composed from torch ops: cross products, quaternion products, banded matrix products and an
    index_add per call."""
    mov = (gid >= 0) & (gid < G)
    g = gid.clamp(0, G - 1).long()
    X = xd[g]
    ct_m, ct_q, ct_s = cts[0], cts[1], cts[2]
    d = posed["means"] - X[:, 9:12]
    om = torch.linalg.cross(d, ct_m)
    q = posed["quats"]
    zero = torch.zeros_like(q[:, 0])
    for k in range(3):
        e = [zero, zero, zero, zero]
        e[1 + k] = zero + 1
        om[:, k] += 0.5 * (ct_q * quat_mul(torch.stack(e, -1), q)).sum(-1)
    if sh:
        c, cb = posed["colors"], cts[3]
        for l in range(1, DEG + 1):
            blk = slice(l * l, (l + 1) ** 2)
            om += torch.einsum("nic,kij,njc->nk", cb[:, blk], gens[l], c[:, blk])
    lam = (ct_m * d).sum(-1) + (ct_s * posed["scales"]).sum(-1)
    add = torch.cat([om, ct_m, lam[:, None]], 1) * mov[:, None]
    v_pose = torch.zeros(G, 7, device=gid.device).index_add_(0, g, add)
    m3 = mov[:, None]
    v_means = torch.where(m3, torch.einsum("nji,nj->ni", X[:, :9].reshape(-1, 3, 3), ct_m), ct_m)
    conj = X[:, 12:16] * torch.tensor([1.0, -1.0, -1.0, -1.0], device=gid.device)
    v_quats = torch.where(m3, quat_mul(conj, ct_q), ct_q)
    v_scales = torch.where(m3, X[:, 16:17] * ct_s, ct_s)
    v_sh = None
    if sh:
        Rr, parts, off = rd[g], [cts[3][:, :1]], 0
        for l in range(1, DEG + 1):
            m = 2 * l + 1
            M = Rr[:, off:off + m * m].reshape(-1, m, m)
            off += m * m
            parts.append(torch.einsum("nkj,nkc->njc", M, cts[3][:, l * l:(l + 1) ** 2]))
        v_sh = torch.where(mov[:, None, None], torch.cat(parts, 1), cts[3])
    return v_pose, v_means, v_quats, v_scales, v_sh


def timed(fns):
    """Mean microseconds per call of each fn, the calls alternating."""
    for _ in range(WARMUP):
        for f in fns:
            f()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)] for _ in fns]
    torch.cuda.synchronize()
    for i in range(CALLS):
        for j, f in enumerate(fns):
            ev[j][i][0].record()
            f()
            ev[j][i][1].record()
    torch.cuda.synchronize()
    return [sum(a.elapsed_time(b) for a, b in e) / CALLS * 1e3 for e in ev]


def main():
    blocks = "--blocks" in sys.argv
    scene = synthetic_scene(N, math.log(0.012), DEG, 0)
    t = scene.to_torch("cuda", DEG)
    rng = np.random.default_rng(0)
    Rs = []
    for _ in range(G):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        Rs.append(q)
    R = torch.tensor(np.stack(Rs), device="cuda", requires_grad=True)
    tr = torch.tensor(rng.normal(size=(G, 3)), device="cuda", requires_grad=True)
    ids = (np.arange(N) * G // N) if blocks else rng.integers(0, G, size=N)
    gid_all = torch.from_numpy(ids.astype(np.int32)).cuda()
    keep = (torch.arange(N, device="cuda") < N // 10) if blocks else (torch.rand(N, device="cuda") < 0.1)
    gid_10 = torch.where(keep, gid_all, torch.full_like(gid_all, -1))
    xd, rd = pack_transforms_torch(R, tr, None, DEG)
    gens = [None] + [torch.tensor(np.stack([sh_generator_matrices(DEG)[k][l] for k in range(3)]), dtype=torch.float32,
                                  device="cuda") for l in range(1, DEG + 1)]
    ws = torch.empty(workspace_bytes(N, G) + 256, dtype=torch.uint8, device="cuda")
    print(f"{N} Gaussians, {G} groups, SH degree {DEG}, group ids {'part by part' if blocks else 'random'}; "
          f"workspace {workspace_bytes(N, G) / 2**20:.1f} MiB")
    for name, gid, sh in (("all moving, SH", gid_all, True), ("all moving, no SH", gid_all, False), ("10 % moving, SH", gid_10, True)):
        posed = transform_gaussians(t, group_ids=gid, rotate_sh=sh, packed=(xd, rd))
        cts = [torch.randn_like(posed[k]) for k in ("means", "quats", "scales")] + ([torch.randn_like(posed["colors"])] if sh else [None])
        out = {}
        raw = lambda: out.update(pose_bwd_raw(posed["means"], posed["quats"], posed["scales"], posed["colors"] if sh else None,
                                              DEG, gid, xd, rd, cts[0], cts[1], cts[2], cts[3], rest=True, out=out, workspace=ws))
        leaf = {k: (v.detach().requires_grad_(True) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in t.items()}
        keys = ("means", "quats", "scales") + (("colors",) if sh else ())

        def through():
            p = pose_gaussians(leaf, R, tr, group_ids=gid, rotate_sh=sh)
            torch.autograd.backward([p[k] for k in keys], [c for c in cts if c is not None])
            for v in (R, tr, *[leaf[k] for k in keys]):
                v.grad = None
        composed = lambda: torch_backward(posed, cts, gid, xd, rd, gens, sh)
        us = timed([raw, through, composed])
        n_mov = int(((gid >= 0) & (gid < G)).sum())
        # posed state, cotangent and rest-pose gradient: 44 B each; SH rows: posed + cotangent + gradient for a moving
        # Gaussian, cotangent + gradient for one that passes through
        need = N * 44 * 3 + (n_mov * 192 * 3 + (N - n_mov) * 192 * 2 if sh else 0)
        print(f"{name}: backward alone {us[0]:.1f} us ({need / 1e6:.0f} MB needed, {need / (us[0] * 1e-6) / PEAK * 100:.0f} % of 8 TB/s); "
              f"forward + backward through pose_gaussians {us[1]:.1f} us; composed from torch ops {us[2]:.1f} us "
              f"({us[2] / us[0]:.1f} x the backward alone)")


if __name__ == "__main__":
    main()
