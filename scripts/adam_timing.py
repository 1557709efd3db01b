"""Time one optimiser step over the five Trainer.KEYS leaves of a 1 M Gaussian / SH 3 scene (59 M floats):
GaussianAdam unmasked and with 100 / 50 / 25 % of the Gaussians visible, against torch.optim.Adam(fused=True,
capturable=True) and torch's default foreach form on tensors of the same shapes.

HIP-event times, one process.  Every variant is warmed up, then timed in `--rounds` windows of `--steps` steps each, the
variants taking turns inside every round so that drift and neighbours hit all of them alike; the table gives the median
window and the min..max spread per step.  Needs a GPU: there is no fallback.

    python scripts/adam_timing.py [--n 1000000] [--steps 50] [--rounds 10] [--out table.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robosimgs_amd import GaussianAdam, Trainer, splatfacto_groups  # noqa: E402

HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12       # B/s: the spec, and the float4-copy rate an MI355X reaches


def leaves(n, seed, dev):
    shapes = {"means": (n, 3), "quats": (n, 4), "scales": (n, 3), "opacities": (n,), "colors": (n, 16, 3)}
    gen = torch.Generator(dev).manual_seed(seed)
    p = {k: torch.randn(s, device=dev, generator=gen).requires_grad_(True) for k, s in shapes.items()}
    for v in p.values():
        v.grad = torch.randn(v.shape, device=dev, generator=gen) * 1e-2
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "adam_timing.py measures on the GPU"
    dev = "cuda"
    n = a.n
    ours, fused, foreach = leaves(n, 0, dev), leaves(n, 0, dev), leaves(n, 0, dev)
    floats = sum(v.numel() for v in ours.values())
    opt = GaussianAdam(splatfacto_groups(ours), eps=1e-15)
    opt_fused = torch.optim.Adam(list(fused.values()), lr=1e-3, eps=1e-15, fused=True, capturable=True)
    opt_foreach = torch.optim.Adam(list(foreach.values()), lr=1e-3, eps=1e-15)
    gen = torch.Generator(dev).manual_seed(1)
    u = torch.rand(n, device=dev, generator=gen)
    radii = {f: ((u < f).to(torch.int32) * 9)[None].contiguous() for f in (1.0, 0.5, 0.25)}
    variants = [("GaussianAdam, unmasked", lambda: opt.step(), 1.0)]
    variants += [(f"GaussianAdam, {int(100 * f)} % visible", (lambda r: lambda: opt.step(visibility=r))(radii[f]), f)
                 for f in (1.0, 0.5, 0.25)]
    variants += [("torch.optim.Adam(fused=True, capturable=True)", lambda: opt_fused.step(), None),
                 ("torch.optim.Adam (default, foreach)", lambda: opt_foreach.step(), None)]
    for _, fn, _ in variants:                  # warm-up: state allocation, code objects
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, fn, _ in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps * 1e3)          # us per step
    nbytes = 7 * 4 * floats                                                  # p, g, m, v read; p, m, v written
    lines = [f"{n} Gaussians, SH 3, {len(Trainer.KEYS)} leaves, {floats / 1e6:.1f} M floats; an unmasked step moves "
             f"{nbytes / 1e9:.2f} GB.  {a.rounds} windows of {a.steps} steps per variant, variants alternating.", "",
             "| variant | median us / step | min .. max | spread | GB/s | of 8 TB/s | of 6.3 TB/s |", "|---|---|---|---|---|---|---|"]
    for name, _, frac in variants:
        t = times[name]
        med = statistics.median(t)
        row = f"| {name} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {100 * (max(t) - min(t)) / med:.1f} % |"
        if frac == 1.0 or frac is None:
            rate = nbytes / (med * 1e-6)
            row += f" {rate / 1e9:.0f} | {100 * rate / HBM_PEAK:.0f} % | {100 * rate / HBM_STREAM:.0f} % |"
        else:
            row += " | | |"
        lines.append(row)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
