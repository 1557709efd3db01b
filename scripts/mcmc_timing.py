"""Time splatfacto-mcmc's refinement on a 1 M Gaussian / SH 3 scene: the per-step noise injection (mgs_mcmc_noise), a
relocation with 5 % of the Gaussians dead and a growth by 5 % (mgs_mcmc_relocate in its two modes), each against a plain
torch statement of the same operation on the same tensors (written below: what a trainer without the library runs).

HIP-event times, one process.  Every variant is warmed up, then timed in `--rounds` windows, the variants taking turns
inside every round so that drift and neighbours hit all of them alike; the table gives the median window and the
min..max spread per call.  Both sides of a pair get the same pre-drawn random numbers (drawing them is not timed), and
both relocations start every call from the same restored opacities and scales (the restore, two copies of 16 MB together,
is inside both timings).  Needs a GPU: there is no fallback.

    python scripts/mcmc_timing.py [--n 1000000] [--steps 500] [--refines 20] [--rounds 10] [--out table.md]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robosimgs_amd import _lib  # noqa: E402
from robosimgs_amd.strategy import KEYS, _Scratch, mcmc_noise, mcmc_relocate  # noqa: E402

HBM_STREAM = 6.3e12        # B/s: the float4-copy rate an MI355X reaches
MIN_O, MAX_RATIO, O_MAX = 0.005, 51, 1.0 - 2.0 ** -23


# ---- the torch statements ----------------------------------------------------------------------------------------------
def torch_noise(means, quats, scales, opacities, z, lam):
    """gsplat's inject_noise_to_position on raw parameters, the two 3 x 3 products written element-wise (as batched
    matmuls -- `(R * s2[:, None, :]) @ R.transpose(1, 2)` and an einsum -- the same statement took 22 ms at 1 M: a million
    3 x 3 GEMMs)."""
    w, x, y, zq = torch.nn.functional.normalize(quats, dim=-1).unbind(-1)
    R = torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - w * zq), 2 * (x * zq + w * y),
                     2 * (x * y + w * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - w * x),
                     2 * (x * zq - w * y), 2 * (y * zq + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    gate = torch.sigmoid(100.0 * ((1.0 - torch.sigmoid(opacities)) - 0.995))
    v = z * (gate * lam)[:, None]
    t = (R * v[:, :, None]).sum(1) * torch.exp(2.0 * scales)            # diag(s^2) R^T v
    means.add_((R * t[:, None, :]).sum(2))                              # R (.)


class TorchRefine:
    """gsplat's relocate_gs / sample_add on raw parameters, with the inverse-CDF draw and the fp64 sum of the library's
    contract so that both sides do the same arithmetic."""

    def __init__(self, dev):
        k = torch.arange(MAX_RATIO, device=dev, dtype=torch.float64)
        comb = torch.zeros(MAX_RATIO, MAX_RATIO, dtype=torch.float64)
        for r in range(1, MAX_RATIO + 1):
            for j in range(r):
                comb[r - 1, j] = math.comb(r, j + 1) * (-1.0) ** j / math.sqrt(j + 1)
        self.coef, self.k1 = comb.to(dev), k + 1

    def draw(self, w, u):
        cdf = torch.cumsum(w.double(), 0)
        return torch.searchsorted(cdf, u.double() * cdf[-1], right=True).clamp_(max=w.shape[0] - 1)

    def new_values(self, logits, log_scales, ratio):
        r = ratio.clamp(max=MAX_RATIO)
        o = torch.sigmoid(logits.double()).clamp(max=O_MAX)
        o_new = -torch.expm1(torch.log1p(-o) / r)
        D = (self.coef[r - 1] * o_new[:, None] ** self.k1).sum(-1)
        kept = o_new.clamp(MIN_O, O_MAX)
        return torch.log(kept / (1 - kept)).float(), log_scales + torch.log(o / D).float()[:, None]

    def relocate(self, P, M, n, u):
        o = torch.sigmoid(P["opacities"][:n])
        dead = o <= MIN_O
        dead_idx = dead.nonzero(as_tuple=True)[0]                         # the host read-back of a dynamic shape
        src = self.draw(torch.where(dead, torch.zeros_like(o), o), u[:dead_idx.shape[0]])
        ratio = torch.bincount(src, minlength=n)[src] + 1
        P["opacities"][src], P["scales"][src] = self.new_values(P["opacities"][src], P["scales"][src], ratio)
        for k in KEYS:
            P[k][dead_idx] = P[k][src]
            for m in M[k]:
                m[src] = 0

    def add(self, P, M, n, n_new, u):
        src = self.draw(torch.sigmoid(P["opacities"][:n]), u[:n_new])
        ratio = torch.bincount(src, minlength=n)[src] + 1
        P["opacities"][src], P["scales"][src] = self.new_values(P["opacities"][src], P["scales"][src], ratio)
        grown = {k: torch.cat([P[k][:n], P[k][src]]) for k in KEYS}        # gsplat rebuilds every tensor
        moments = {k: tuple(torch.cat([m[:n], torch.zeros_like(m[:n_new])]) for m in M[k]) for k in KEYS}
        return grown, moments


def scene(n, cap, dev, seed):
    gen = torch.Generator(dev).manual_seed(seed)
    shapes = {"means": (3,), "quats": (4,), "scales": (3,), "opacities": (), "colors": (16, 3)}
    P = {k: torch.randn((cap, *s), device=dev, generator=gen) for k, s in shapes.items()}
    P["scales"] = P["scales"] * 0.4 + math.log(0.02)
    P["opacities"] = P["opacities"] * 1.5
    P["opacities"][:n][torch.rand(n, device=dev, generator=gen) < 0.05] = -7.0       # 5 % dead
    M = {k: (torch.rand_like(v) * 1e-2, torch.rand_like(v) * 1e-4) for k, v in P.items()}
    return P, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=500, help="noise calls per window")
    ap.add_argument("--refines", type=int, default=20, help="relocate / add calls per window")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mcmc_timing.py measures on the GPU"
    dev = "cuda"
    n, n_new = a.n, a.n // 20
    cap = n + n_new
    ours, ours_m = scene(n, cap, dev, 0)
    theirs, theirs_m = scene(n, cap, dev, 0)
    saved = {k: ours[k].clone() for k in ("opacities", "scales")}
    gen = torch.Generator(dev).manual_seed(1)
    z = torch.randn(n, 3, device=dev, generator=gen)
    u = torch.rand(n, device=dev, generator=gen)
    lam = 5e5 * 1.6e-4 * 1e-3           # small: hundreds of calls must not carry the means away
    state = torch.tensor([100, 0], dtype=torch.int32, device=dev)
    scratch = _Scratch(cap, dev)
    ref = TorchRefine(dev)
    views = lambda P: [P[k][:n] for k in ("means", "quats", "scales", "opacities")]

    def restore(P):
        for k, v in saved.items():
            P[k].copy_(v)

    def our_relocate():
        restore(ours)
        mcmc_relocate(_lib.MCMC_RELOCATE, n, 0, ours, ours_m, MIN_O, u, scratch)

    def their_relocate():
        restore(theirs)
        ref.relocate(theirs, theirs_m, n, u)

    def our_add():
        restore(ours)
        mcmc_relocate(_lib.MCMC_ADD, n, n_new, ours, ours_m, MIN_O, u, scratch)

    def their_add():
        restore(theirs)
        ref.add(theirs, theirs_m, n, n_new, u)

    variants = [
        ("noise: mgs_mcmc_noise (device counter and schedule)", a.steps,
         lambda: mcmc_noise(*views(ours), z, 5e5 * 1e-3, 1.6e-4, 1.6e-6, 30000, state)),
        ("noise: torch statement", a.steps, lambda: torch_noise(*views(theirs), z, lam)),
        ("relocate, 5 % dead: mgs_mcmc_relocate", a.refines, our_relocate),
        ("relocate, 5 % dead: torch statement", a.refines, their_relocate),
        ("add 5 %: mgs_mcmc_relocate", a.refines, our_add),
        ("add 5 %: torch statement (rebuilds the tensors)", a.refines, their_add),
        ("(the restore of opacities and scales inside the four rows above)", a.refines, lambda: restore(ours)),
    ]
    for _, _, fn in variants:                  # warm-up: code objects, workspaces, the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, calls, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls * 1e3)            # us per call
    n_dead = int((torch.sigmoid(saved["opacities"][:n]) <= MIN_O).sum())
    noise_bytes = 68 * n                                                     # 56 B read, 12 B written per Gaussian
    lines = [f"{n} Gaussians, SH 3, {n_dead} dead ({100 * n_dead / n:.1f} %), {n_new} added.  {a.rounds} windows per "
             f"variant ({a.steps} noise calls, {a.refines} refinement calls each), variants alternating.  The noise "
             f"launch moves {noise_bytes / 1e6:.0f} MB.", "",
             "| variant | median us / call | min .. max | spread | GB/s | of 6.3 TB/s |", "|---|---|---|---|---|---|"]
    for name, _, _ in variants:
        t = times[name]
        med = statistics.median(t)
        row = f"| {name} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {100 * (max(t) - min(t)) / med:.1f} % |"
        if name.startswith("noise"):
            rate = noise_bytes / (med * 1e-6)
            row += f" {rate / 1e9:.0f} | {100 * rate / HBM_STREAM:.0f} % |"
        else:
            row += " | |"
        lines.append(row)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
