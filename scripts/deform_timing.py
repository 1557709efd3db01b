"""Cost of particle-driven deformation (include/mgs_deform.h, csrc/deform.hip) at the size the issue names: a scene of 1 M
Gaussians of which 200 k (the soft object, `select`) are bound to 50 k particles.

  bind     mgs_deform_bind (two launches), once per object; the pair rate n_bound x m / time against the vector-issue
           estimate (VALU_PER_PAIR instructions per pair: 3 subtractions, 1 multiply, 2 fma, 1 compare; one wave
           instruction per 2 cycles on each of 256 x 4 SIMDs at 2.4 GHz)
  apply    mgs_deform_apply, rigid and affine, over the whole scene (unbound Gaussians pass through); "needed" = the bytes
           the algorithm moves, from the shapes, and their share of the MI355X's 8 TB/s
  + SH     mgs_deform_apply_sh (include/mgs_deform_sh.h), degree 3, copy_unbound = 0: 384 B more per bound Gaussian (its
           192-byte row read and written).  --parent-lib <libmgs.so of the parent commit>: that build's mgs_deform_apply
           alternates with this one's in the same loop (the path without SH must not have slowed).  For scale,
           mgs_transform_gaussians (host-made matrices) on the same 200 k rows as one group, with and without SH
  torch    the only baseline there is -- the parent commit has no such path: cdist + topk in chunks, then batched moments
           and torch.linalg.svd
  frames   FrameRenderer frames per second at 1 M Gaussians, 1920 x 1080, three frames in flight, with and without deform=

Device events, a warm-up, the variants alternating call by call in one process.  Needs a GPU: there is no fallback.

    python scripts/deform_timing.py [--rounds 10] [--frames 120] [--out table.md] [--resources] [--parent-lib PATH]
"""
import argparse
import ctypes
import math
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_PAIR = 7.0
PEAK_PAIRS = 256 * 4 * 2.4e9 / 2 * 64 / VALU_PER_PAIR
N, N_SOFT, M = 1_000_000, 200_000, 50_000
HBM = 8e12


def resources():
    from robosimgs_amd.csrc import build as B
    src = os.path.join(B.HERE, "deform.hip")
    cmd = [B._hipcc(), *B.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "") for ln in r.stderr.splitlines()
             if "remark:" in ln]
    return [ln.split(":0: ", 1)[-1].strip() for ln in lines]


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def torch_bind(means, parts, chunk=4096):
    """cdist + topk in chunks, then the weights, offsets and the inverse moment matrix, in torch ops."""
    import torch
    idx, d2 = [], []
    for s in range(0, means.shape[0], chunk):
        d = torch.cdist(means[s:s + chunk], parts).square_()
        v, i = torch.topk(d, 8, dim=1, largest=False)
        idx.append(i)
        d2.append(v)
    idx, d2 = torch.cat(idx), torch.cat(d2)
    w = torch.softmax(-d2 / d2[:, 7:8], dim=1)
    X = parts[idx]
    Xbar = (w[..., None] * X).sum(1)
    r = X - Xbar[:, None]
    Q = torch.einsum("nk,nka,nkb->nab", w, r, r)
    return idx, w, w[..., None] * r, means - Xbar, torch.linalg.pinv(Q)


def torch_apply(bound, now, quats, affine):
    """The per-frame part from torch ops: gather, weighted moments, a batched SVD."""
    import torch
    idx, w, p, d0, Qinv = bound
    x = now[idx]
    xbar = (w[..., None] * x).sum(1)
    P = torch.einsum("nka,nkb->nab", x - xbar[:, None], p)
    if affine:
        A = P @ Qinv
        return xbar + (A @ d0[..., None])[..., 0], A
    U, _, Vh = torch.linalg.svd(P)
    R = U @ Vh
    return xbar + (R @ d0[..., None])[..., 0], R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--frames", type=int, default=120, help="frames per timed block of the FrameRenderer comparison")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="only print the compiler's resource report (needs no GPU)")
    ap.add_argument("--parent-lib", default=None, help="a libmgs.so built from the parent commit: its mgs_deform_apply is timed too")
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
    from robosimgs_amd import FrameRenderer, _lib, camera_ring, deform as D, synthetic_scene, transform_gaussians
    from robosimgs_amd.transform import pack_transforms
    parent = None
    if a.parent_lib:                       # (not _lib._load: the parent has no mgs_deform_apply_sh to bind)
        parent = ctypes.CDLL(a.parent_lib)
        parent.mgs_deform_apply.argtypes, parent.mgs_deform_apply.restype = _lib._DEFORM_SIGNATURES["mgs_deform_apply"]

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

    def bind_and_apply(label, tensors, soft):
        means = tensors["means"]
        # ---- bind ---------------------------------------------------------------------------------------------------------------
        sel = soft.to(torch.uint8)
        idx = torch.empty((8, N), dtype=torch.int32, device=dev)
        w = torch.empty((8, N), device=dev)
        p = torch.empty((8, 3, N), device=dev)
        rs = torch.empty((12, N), device=dev)
        fl = torch.empty((N,), dtype=torch.uint8, device=dev)
        ws = torch.empty(D.bind_workspace_bytes(N, M) + 256, dtype=torch.uint8, device=dev)
        bind = lambda: D.deform_bind_raw(means, rest, sel, math.inf, idx, w, p, rs, fl, workspace=ws)
        soft_means = means[soft].contiguous()
        tb = lambda: torch_bind(soft_means, rest)
        for _ in range(2):
            bind()
        tb()
        torch.cuda.synchronize()
        t_bind, t_tb = [], []
        for k in range(a.rounds):
            t_bind.append(timed(bind, 1))
            if k < 3:                                                          # the torch composition: three calls are enough
                t_tb.append(timed(tb, 1))
        binding = D.ParticleBinding(idx, w, p, rs, fl, N, M, rest)
        flags = np.bincount(fl.cpu().numpy(), minlength=8)
        pairs = float(n_soft) * M
        mb = statistics.median(t_bind)
        say(f"{label} -- bind: {n_soft} bound of {N} Gaussians x {M} particles: mgs_deform_bind {mb / 1e3:.2f} ms ({min(t_bind) / 1e3:.2f} .. "
            f"{max(t_bind) / 1e3:.2f}), {pairs / (mb * 1e-6):.3g} pairs/s = {pairs / (mb * 1e-6) / PEAK_PAIRS:.1%} of the vector-issue "
            f"estimate; torch cdist + topk + moments {statistics.median(t_tb) / 1e3:.1f} ms; flags: unbound {flags[1]}, flat "
            f"{flags[2] + flags[6]}, thin {flags[4] + flags[6]}")

        # ---- apply --------------------------------------------------------------------------------------------------------------
        outs = {k: torch.empty_like(tensors[k]) for k in ("means", "quats", "scales")}
        st = torch.zeros(N, dtype=torch.uint8, device=dev)
        bound_t = torch_bind(soft_means, rest)
        soft_q = tensors["quats"][soft].contiguous()
        outs_sh = dict({k: torch.empty_like(v) for k, v in outs.items()}, colors=tensors["colors"].clone())
        gid = torch.where(soft, 0, -1).to(torch.int32)
        ang = 0.3
        xr = pack_transforms([[[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1]]], [[0.01, 0, 0]], None, 3)
        packed = (torch.from_numpy(xr[0]).to(dev), torch.from_numpy(xr[1]).to(dev))
        outs_t = dict(tensors, colors=tensors["colors"].clone(), **{k: torch.empty_like(v) for k, v in outs.items()})

        def raw_apply(L, mode):              # mgs_deform_apply as the C ABI has it: the same call path for both builds
            rc = L.mgs_deform_apply(N, tensors["means"].data_ptr(), tensors["quats"].data_ptr(), tensors["scales"].data_ptr(),
                                         idx.data_ptr(), w.data_ptr(), p.data_ptr(), rs.data_ptr(), fl.data_ptr(), mode, M,
                                         now.data_ptr(), outs["means"].data_ptr(), outs["quats"].data_ptr(),
                                         outs["scales"].data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
        calls = {
            "rigid": lambda: D.deform_gaussians(tensors, binding, now, mode="rigid", out=outs, status=st),
            "affine": lambda: D.deform_gaussians(tensors, binding, now, mode="affine", out=outs, status=st),
            "rigid + SH": lambda: D.deform_gaussians(tensors, binding, now, mode="rigid", out=outs_sh, status=st, rotate_sh=True,
                                                     copy_unbound=False),
            "affine + SH": lambda: D.deform_gaussians(tensors, binding, now, mode="affine", out=outs_sh, status=st, rotate_sh=True,
                                                      copy_unbound=False),
            "transform": lambda: transform_gaussians(tensors, group_ids=gid, rotate_sh=False, out=outs_t, packed=packed),
            "transform + SH": lambda: transform_gaussians(outs_t, group_ids=gid, rotate_sh=True, out=outs_t, packed=packed),
            "torch rigid": lambda: torch_apply(bound_t, now, soft_q, False),
            "torch affine": lambda: torch_apply(bound_t, now, soft_q, True),
        }
        if parent is not None:
            # (rigid: this build follows the parent's; affine: the parent's follows this build's -- whoever runs second finds
            # the binding arrays in the caches)
            calls["parent rigid"] = lambda: raw_apply(parent, 0)
            calls["this rigid"] = lambda: raw_apply(_lib.lib(), 0)
            calls["this affine"] = lambda: raw_apply(_lib.lib(), 1)
            calls["parent affine"] = lambda: raw_apply(parent, 1)
        for k, fn in calls.items():
            for _ in range(1 if k.startswith("torch") else 3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for rnd in range(a.rounds):
            for k, fn in calls.items():
                if k.startswith("torch") and rnd >= 3:
                    continue
                t[k].append(timed(fn, 1 if k.startswith("torch") else 5))
        status = {}
        for k in ("rigid", "affine"):
            calls[k]()
            status[k] = np.bincount(st.cpu().numpy(), minlength=9)
        # bytes from the shapes: every Gaussian reads its flag, 40 B of state and writes 40 B + 1 status byte; a bound one also
        # reads idx 32, w 28 (rows 1..7), p 84, d0 12 (affine: + Q^-1 24) and gathers 8 positions of 12 B
        base = N * (1 + 40 + 40 + 1)
        need = {"rigid": base + n_soft * (32 + 28 + 84 + 12 + 96), "affine": base + n_soft * (32 + 28 + 84 + 36 + 96)}
        for k in ("rigid", "affine"):                                          # a bound Gaussian's 192-byte row, read and written
            need[k + " + SH"] = need[k] + n_soft * 384
        say()
        say(f"{label}:")
        say("| apply | us (min .. max) | needed | share of 8 TB/s | composed from torch ops, us | status: deformed / unbound / fell back / thin |")
        say("|---|---|---|---|---|---|")
        for k in ("rigid", "affine"):
            med = statistics.median(t[k])
            s = status[k]
            say(f"| {k} | {med:.1f} ({min(t[k]):.1f} .. {max(t[k]):.1f}) | {need[k] / 1e6:.0f} MB | {need[k] / (med * 1e-6) / HBM:.1%} | "
                f"{statistics.median(t['torch ' + k]):.0f} | {s[0]} / {s[1]} / {s[2]} / {s[4]} |")
        for k in ("rigid + SH", "affine + SH"):
            med = statistics.median(t[k])
            say(f"| {k} | {med:.1f} ({min(t[k]):.1f} .. {max(t[k]):.1f}) | {need[k] / 1e6:.0f} MB | {need[k] / (med * 1e-6) / HBM:.1%} | | |")
        for k in ("parent rigid", "parent affine"):
            if k in t:
                own = t["this " + k.split()[1]]
                say(f"| {k} (mgs_deform_apply of the parent commit's build, called through ctypes) | {statistics.median(t[k]):.1f} "
                    f"({min(t[k]):.1f} .. {max(t[k]):.1f}) | | | | this build's, called the same way: {statistics.median(own):.1f} "
                    f"({min(own):.1f} .. {max(own):.1f}), median "
                    f"{'ABOVE' if statistics.median(own) > max(t[k]) else 'below' if statistics.median(own) < min(t[k]) else 'inside'} "
                    f"the parent's spread |")
        md = {k: statistics.median(t[k]) for k in t}
        say(f"| mgs_transform_gaussians, the same {n_soft} rows as one group | {md['transform']:.1f} ({min(t['transform']):.1f} .. "
            f"{max(t['transform']):.1f}) | | | | + SH (in place, host-made matrices): {md['transform + SH']:.1f} "
            f"({min(t['transform + SH']):.1f} .. {max(t['transform + SH']):.1f}) |")
        say(f"SH - no SH: deform rigid {md['rigid + SH'] - md['rigid']:+.1f} us, deform affine {md['affine + SH'] - md['affine']:+.1f} us, "
            f"transform {md['transform + SH'] - md['transform']:+.1f} us")

        return binding

    from robosimgs_amd.pipeline import locality_order
    order = locality_order(means)
    in_order = {k: (v.index_select(0, order).contiguous() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == N else v)
                for k, v in tensors.items()}
    binding = bind_and_apply("scene as given (the soft Gaussians scattered through the index range)", tensors, soft)
    bind_and_apply("scene in Morton order (FrameRenderer's own copy)", in_order, soft.index_select(0, order))
    say()

    # ---- frames per second ----------------------------------------------------------------------------------------------------
    W, H = 1920, 1080
    cams = camera_ring(a.frames, W, H)
    packed = [FrameRenderer.pack_camera(c.viewmat(), c.K) for c in cams]
    kw = dict(render_mode="RGB", frames_in_flight=3, sizing_camera=(cams[0].viewmat(), cams[0].K), capacity_margin=2.0)
    renderers = {"static": FrameRenderer(tensors, W, H, **kw), "deform": FrameRenderer(tensors, W, H, deform=binding, **kw),
                 "deform + SH": FrameRenderer(tensors, W, H, deform=binding, deform_rotate_sh=True, **kw)}
    feeds = [(rest + 0.01 * torch.sin(7.0 * rest.roll(1, 1) + 0.1 * k)).contiguous() for k in range(8)]

    def block(name):
        r = renderers[name]
        tickets, nxt = [], 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.frames):
            while nxt < a.frames and len(tickets) < r.n_slots:
                extra = dict(particles=feeds[nxt % len(feeds)]) if name.startswith("deform") else {}
                tickets.append(r.submit(packed[nxt], None, **extra))
                nxt += 1
            tk = tickets.pop(0)
            r.fetch(tk, check=False)
            r.release(tk)
        torch.cuda.synchronize()
        return a.frames / (time.perf_counter() - t0)
    for name in renderers:
        block(name)
    fps = {k: [] for k in renderers}
    for _ in range(max(3, a.rounds // 2)):
        for name in renderers:
            fps[name].append(block(name))
    assert all(r.isect_status_max() == 0 for r in renderers.values())
    say()
    say("| FrameRenderer, 1 M Gaussians, 1920 x 1080, 3 in flight | frames/s (min .. max) |")
    say("|---|---|")
    for name, v in fps.items():
        say(f"| {name} | {statistics.median(v):.0f} ({min(v):.0f} .. {max(v):.0f}) |")


if __name__ == "__main__":
    main()
