"""Cost of fitting a hinge (include/mgs_hinge.h, csrc/hinge.hip) at two sizes:
  open box     the reference project's lid and body meshes, 4,410 x 8,416 vertices (tests/golden/hinge_openbox.npz)
  two boxes    2*10^5 x 8*10^5 uniform points in two unit boxes that touch in the plane x = 0: parts that are Gaussian sets

Whole call: HIP-event time of mgs_hinge_fit (one memset node and four launches) on buffers that stay put; every shape is
warmed up, then timed in `--rounds` windows of `--reps` calls; the table gives the median window and the min..max spread,
and the pair rate 2 n_a n_b / time (both directions are walked) against the vector-issue estimate: VALU_PER_PAIR
instructions per pair (3 subtractions, 1 multiply, 2 fma and half a v_min3 as built), one wave instruction per 2 cycles on
each of 256 x 4 SIMDs at 2.4 GHz.
Per kernel (`--trace DIR`): the same calls in a child process under `rocprofv3 --kernel-trace`, a run of its own; the
median duration of every launch of a call, in launch order (nn A->B, nn B->A, moments, final).
For context only, on the host: scipy's k-d tree on the same inputs where scipy is installed (what the reference project
runs), else the fp64 brute force of tests/hinge_ref.py at the open box's size.
`--resources`: the compiler's resource report of csrc/hinge.hip (needs no GPU).  Everything else needs a GPU: there is no
fallback.

    python scripts/hinge_timing.py [--rounds 12] [--reps 5] [--trace DIR] [--out table.md] [--resources]
"""
import argparse
import csv
import glob
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALU_PER_PAIR = 6.5
PEAK_PAIRS = 256 * 4 * 2.4e9 / 2 * 64 / VALU_PER_PAIR       # pairs per second at the vector-issue limit
KERNELS = ["nn A->B", "nn B->A", "moments", "final"]
CHILD_WARM, CHILD_CALLS = 3, 12


def resources():
    from robosimgs_amd.csrc import build as B
    src = os.path.join(B.HERE, "hinge.hip")
    cmd = [B._hipcc(), *B.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "") for ln in r.stderr.splitlines()
             if "remark:" in ln]
    return [ln.split(":0: ", 1)[-1].strip() for ln in lines]


def shapes():
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "hinge_openbox.npz"))
    rng = np.random.default_rng(0)
    a = rng.random((200_000, 3)).astype(np.float32)
    b = rng.random((800_000, 3)).astype(np.float32)
    b[:, 0] -= 1.0                                           # [-1, 0] x [0, 1]^2 against [0, 1]^3
    return {"open box": (g["lid"], g["body"]), "two boxes": (a, b)}


class Call:
    def __init__(self, a, b):
        import torch
        from robosimgs_amd import articulation as art
        dev = torch.device("cuda")
        self.a, self.b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        self.ca = torch.empty(len(a), dtype=torch.uint8, device=dev)
        self.cb = torch.empty(len(b), dtype=torch.uint8, device=dev)
        self.joint = torch.empty(art.JOINT_DOUBLES, dtype=torch.float64, device=dev)
        self.ws = art.hinge_workspace(len(a), len(b), dev)
        self.fit = art.hinge_fit_raw

    def __call__(self):
        self.fit(self.a, self.b, 0.01, self.ca, self.cb, self.joint, workspace=self.ws)


def child():
    """What runs under the profiler: CHILD_WARM + CHILD_CALLS calls per shape, in the order of shapes()."""
    import torch
    for a, b in shapes().values():
        call = Call(a, b)
        for _ in range(CHILD_WARM + CHILD_CALLS):
            call()
            torch.cuda.synchronize()


def per_kernel(trace_dir):
    """{shape: {kernel: (median us, min, max)}} from a rocprofv3 kernel trace of child()."""
    os.makedirs(trace_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "-o", "hinge", "--", sys.executable,
           os.path.abspath(__file__), "--child"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    rows = [r for r in csv.DictReader(open(files[0])) if "hinge_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_shape = 4 * (CHILD_WARM + CHILD_CALLS)
    names = list(shapes())
    assert len(rows) == per_shape * len(names), (len(rows), per_shape)
    out = {}
    for s, name in enumerate(names):
        block = rows[s * per_shape + 4 * CHILD_WARM:(s + 1) * per_shape]
        out[name] = {}
        for k, kernel in enumerate(KERNELS):
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in block[k::4]]
            assert all(("hinge_nn", "hinge_nn", "hinge_moments", "hinge_final")[k] in r["Kernel_Name"] for r in block[k::4])
            out[name][kernel] = (statistics.median(us), min(us), max(us))
    return out


def host_context(name, a, b):
    import numpy as np
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        if len(a) * len(b) > 1e8:
            return "host: not measured (no scipy; the fp64 brute force is out of reach at this size)"
        import hinge_ref
        t0 = time.perf_counter()
        hinge_ref.fit(a, b, 0.01)
        return f"host: {1e3 * (time.perf_counter() - t0):.0f} ms, fp64 NumPy brute force (tests/hinge_ref.py)"
    t0 = time.perf_counter()
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    cKDTree(b64).query(a64)
    cKDTree(a64).query(b64)
    return f"host: {1e3 * (time.perf_counter() - t0):.0f} ms, two scipy k-d trees built and queried (one thread)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--trace", default=None, help="directory for a rocprofv3 kernel trace of a child run: per-kernel times")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="only print the compiler's resource report")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
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
    if a.child:
        return child()
    import torch
    assert a.rounds >= 10, "a median of at least 10 windows"
    say(f"{torch.cuda.get_device_name(0)} on {platform.node()}, torch {torch.__version__}; vector-issue estimate "
        f"{PEAK_PAIRS:.3g} pairs/s at {VALU_PER_PAIR} instructions per pair")
    rows = []
    for name, (pa, pb) in shapes().items():
        call = Call(pa, pb)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        record = call.joint.cpu().numpy()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
        assert call.joint.cpu().numpy().tobytes() == record.tobytes(), "the record changed between runs"
        pairs = 2.0 * len(pa) * len(pb)
        med = statistics.median(us)
        rows.append((name, len(pa), len(pb), med, min(us), max(us), pairs / (med * 1e-6)))
        say(f"{name}: {len(pa)} x {len(pb)}, mgs_hinge_fit {med:.1f} us ({min(us):.1f} .. {max(us):.1f}), "
            f"{pairs / (med * 1e-6):.3g} pairs/s = {pairs / (med * 1e-6) / PEAK_PAIRS:.1%} of the estimate; contact "
            f"{int(record[8])} + {int(record[9])}, min_distance {record[7]:.3g}, axis_confidence {record[6]:.4f}")
        say(f"  {host_context(name, pa, pb)}")
        del call
    say()
    say("| shape | n_a x n_b | mgs_hinge_fit us (min .. max) | pairs/s | of the vector-issue estimate |")
    say("|---|---|---|---|---|")
    for name, na, nb, med, lo, hi, rate in rows:
        say(f"| {name} | {na} x {nb} | {med:.1f} ({lo:.1f} .. {hi:.1f}) | {rate:.3g} | {rate / PEAK_PAIRS:.1%} |")
    if a.trace:
        table = per_kernel(a.trace)
        say()
        say("| shape | " + " | ".join(f"{k} us (min .. max)" for k in KERNELS) + " |")
        say("|---|" + "---|" * len(KERNELS))
        for name, t in table.items():
            say(f"| {name} | " + " | ".join(f"{t[k][0]:.1f} ({t[k][1]:.1f} .. {t[k][2]:.1f})" for k in KERNELS) + " |")


if __name__ == "__main__":
    main()
