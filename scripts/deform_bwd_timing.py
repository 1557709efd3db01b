"""Cost of the backward of particle-driven deformation (include/mgs_deform_bwd.h, csrc/deform.hip) on the scene of
scripts/deform_timing.py: 1 M Gaussians of which 200 k (the soft object) are bound to 50 k particles, as given and in
Morton order.

  forward   mgs_deform_apply, rigid, the yardstick: the backward's first launch does the forward's Jacobi solve plus one
            3 x 3 solve
  backward  mgs_deform_apply_bwd (two launches) with all three cotangents, with and without the rest gradients
  torch     the same gradients from torch autograd: gather, batched moments, torch.linalg.svd, and index_add_ in the
            backward of the gather (the bound 200 k rows only)
  transpose building the transposed binding (a stable sort and a searchsorted), once per binding

Device events, a warm-up, the variants alternating call by call in one process; the median with its range.  Needs a GPU:
there is no fallback.

    python scripts/deform_bwd_timing.py [--rounds 10] [--out table.md] [--resources]
"""
import argparse
import math
import os
import platform
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, N_SOFT, M = 1_000_000, 200_000, 50_000
HBM = 8e12


def resources():
    """The compiler's resource report of the two backward kernels (needs no GPU)."""
    from robosimgs_amd.csrc import build as B
    src = os.path.join(B.HERE, "deform.hip")
    cmd = [B._hipcc(), *B.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip()
             for ln in r.stderr.splitlines() if "remark:" in ln]
    out, keep = [], False
    for ln in lines:
        if ln.startswith("Function Name"):
            keep = "deform_apply_bwd_kernel" in ln or "deform_scatter_kernel" in ln or "deform_apply_kernelILb0" in ln
        if keep:
            out.append(ln)
    return out


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def torch_forward(idx, w, p, d0, q, now):
    """The rigid forward of the bound rows from torch ops (autograd records it): means and the rotation."""
    import torch
    x = now[idx]                                                            # the gather: index_add_ in its backward
    xbar = (w[..., None] * x).sum(1)
    P = torch.einsum("nka,nkb->nab", x - xbar[:, None], p)
    U, _, Vh = torch.linalg.svd(P)
    R = U @ Vh
    return xbar + (R @ d0[..., None])[..., 0], R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="only print the compiler's resource report (needs no GPU)")
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
    from robosimgs_amd import deform as D, synthetic_scene
    from robosimgs_amd.pipeline import locality_order

    dev = torch.device("cuda")
    say(f"{torch.cuda.get_device_name(0)} on {platform.node()}, torch {torch.__version__}")
    g = synthetic_scene(N, math.log(0.01), 3, 1)
    tensors = g.to_torch(dev, 3)
    means = tensors["means"]
    rad = (means - means.mean(0)).norm(dim=1)
    soft = rad <= torch.kthvalue(rad, N_SOFT).values                       # the 200 k Gaussians nearest the centre
    rng = torch.Generator(device="cpu").manual_seed(0)
    pick = torch.nonzero(soft)[:, 0][torch.randperm(int(soft.sum()), generator=rng)[:M].to(dev)]
    rest = (means[pick] + 0.002 * torch.randn(M, 3, generator=rng).to(dev)).contiguous()
    now = (rest + 0.01 * torch.sin(7.0 * rest.roll(1, 1))).contiguous()
    n_soft = int(soft.sum())

    def measure(label, tensors, soft):
        binding = D.bind_particles(tensors["means"], rest, select=soft)
        t_tr = []
        for _ in range(3):
            binding._transposed = None
            t_tr.append(timed(binding.transposed, 1))
        t_start, _ = binding.transposed()
        seg = (t_start[1:] - t_start[:-1]).cpu().numpy()
        outs = {k: torch.empty_like(tensors[k]) for k in ("means", "quats", "scales")}
        st = torch.zeros(N, dtype=torch.uint8, device=dev)
        bst = torch.zeros(N, dtype=torch.uint8, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        ct = [torch.randn(N, c, device=dev, generator=gen) for c in (3, 4, 3)]
        res = {"v_particles": torch.empty(M, 3, device=dev), "v_means": torch.empty(N, 3, device=dev),
               "v_quats": torch.empty(N, 4, device=dev), "v_scales": torch.empty(N, 3, device=dev)}
        ws = torch.empty(D.apply_bwd_workspace_bytes(N) + 256, dtype=torch.uint8, device=dev)
        quats = tensors["quats"]
        # the torch composition on the bound rows
        rows = torch.nonzero(soft)[:, 0]
        t_idx = binding.idx[:, rows].t().long().contiguous()
        t_w = binding.w[:, rows].t().contiguous()
        t_p = binding.p[:, :, rows].permute(2, 0, 1).contiguous()
        t_d0 = binding.rest[0:3, rows].t().contiguous()
        t_ct = ct[0][rows].contiguous()

        def torch_both():
            x = now.clone().requires_grad_(True)
            mu, _ = torch_forward(t_idx, t_w, t_p, t_d0, None, x)
            (mu * t_ct).sum().backward()
            return x.grad

        calls = {
            "forward": lambda: D.deform_gaussians(tensors, binding, now, mode="rigid", out=outs, status=st),
            "backward": lambda: D.deform_apply_bwd_raw(quats, binding, now, st, *ct, out=res, bwd_status=bst, workspace=ws),
            "backward, particles only": lambda: D.deform_apply_bwd_raw(quats, binding, now, st, *ct, rest=False,
                                                                       out={"v_particles": res["v_particles"]}, workspace=ws),
            "torch": torch_both,
        }
        for k, fn in calls.items():
            for _ in range(1 if k == "torch" else 3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for rnd in range(a.rounds):
            for k, fn in calls.items():
                if k == "torch" and rnd >= 3:
                    continue
                t[k].append(timed(fn, 1 if k == "torch" else 5))
        guard = int(bst.sum().item())
        status = np.bincount(st.cpu().numpy(), minlength=9)
        # bytes from the shapes.  launch 1: every Gaussian reads its flag, status and 40 B of cotangents and writes 96 B of
        # contributions (+ 40 B of rest gradients); a bound one also reads idx 32, w 28, p 84, d0 12, q 16 and gathers 8 x 12 B.
        # launch 2: every entry of a bound Gaussian is read (4 B) with its 12 B of contributions; 12 B per particle written.
        need1 = N * (1 + 1 + 40 + 96) + n_soft * (32 + 28 + 84 + 12 + 16 + 96)
        need2 = 8 * n_soft * (4 + 12) + M * (8 + 12)
        need = {"backward": need1 + N * 40 + need2, "backward, particles only": need1 + need2}
        say()
        say(f"{label}: {n_soft} bound of {N} Gaussians, {M} particles; referents per particle {seg.min()} .. {seg.max()}, "
            f"mean {seg.mean():.1f}; forward status deformed / unbound / thin {status[0]} / {status[1]} / {status[4]}; guarded {guard}; "
            f"transposed binding built in {statistics.median(t_tr) / 1e3:.2f} ms")
        say("| call | us (min .. max) | needed | share of 8 TB/s | against the forward |")
        say("|---|---|---|---|---|")
        fwd = statistics.median(t["forward"])
        for k in calls:
            med = statistics.median(t[k])
            nb = need.get(k)
            say(f"| {k} | {med:.1f} ({min(t[k]):.1f} .. {max(t[k]):.1f}) | {'' if nb is None else f'{nb / 1e6:.0f} MB'} | "
                f"{'' if nb is None else f'{nb / (med * 1e-6) / HBM:.1%}'} | {med / fwd:.2f} x |")

    order = locality_order(means)
    in_order = {k: (v.index_select(0, order).contiguous() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == N else v)
                for k, v in tensors.items()}
    measure("scene as given (the soft Gaussians scattered through the index range)", tensors, soft)
    measure("scene in Morton order (FrameRenderer's own copy)", in_order, soft.index_select(0, order))


if __name__ == "__main__":
    main()
