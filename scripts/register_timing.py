"""Cost of register_points (include/mgs_register.h, csrc/register.hip) at the bench scene's size: the 10^6 means of
synthetic_scene(10^6, log 0.012, seed 0) as the source, moved by a small similarity, against 2*10^5 of them (jittered) as the
target, max_distance 2 % of the 6-unit extent.

Whole calls: HIP-event time of mgs_register_icp on buffers that stay put, with iterations 0 (grid build, one query, the
result), 1 and 30 (tol 0: nothing stops early); every shape is warmed up, then timed in `--rounds` windows of `--reps`
calls; median and min..max.  From them: one iteration = (t30 - t0) / 30, grid build = t0 - one iteration (the final pass of
a call is one query and one solve, like an iteration).
Per kernel (`--trace DIR`): the 30-iteration call in a child process under `rocprofv3 --kernel-trace`, a run of its own;
the median duration of every kernel by name.
The yardstick is the parent's only nearest-neighbour path: mgs_hinge_fit on the same two sets walks both directions by brute
force, 2 n_s n_t pairs; its time per pair against the grid query's time per source point gives the pair count at which the
two meet.  `--skip-hinge` leaves it out (it takes most of the run).  Everything needs a GPU: there is no fallback.

    python scripts/register_timing.py [--rounds 10] [--reps 3] [--trace DIR] [--out table.md] [--skip-hinge]
"""
import argparse
import csv
import glob
import os
import platform
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SOURCE, N_TARGET, EXTENT, MD_FRACTION = 1_000_000, 200_000, 6.0, 0.02
CHILD_WARM, CHILD_CALLS = 2, 5


def sets():
    import math
    import numpy as np
    from robosimgs_amd import synthetic_scene
    means = synthetic_scene(N_SOURCE, math.log(0.012), 0, seed=0).means.astype(np.float64)
    rng = np.random.default_rng(1)
    target = means[rng.permutation(N_SOURCE)[:N_TARGET]] + rng.normal(0, 0.002, (N_TARGET, 3))
    a = np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(0.5)
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    source = ((means - [0.01, -0.02, 0.015]) @ R) / 1.004          # the pre-image of the means under (1.004, R, t)
    return source.astype(np.float32), target.astype(np.float32), MD_FRACTION * EXTENT


class Call:
    def __init__(self, source, target, md, iterations):
        import torch
        from robosimgs_amd import registration as reg
        dev = torch.device("cuda")
        self.s, self.t, self.md, self.its = torch.from_numpy(source).to(dev), torch.from_numpy(target).to(dev), md, iterations
        self.c = torch.empty(len(source), dtype=torch.int32, device=dev)
        self.d2 = torch.empty(len(source), dtype=torch.float32, device=dev)
        self.hist = torch.zeros((iterations, 4), dtype=torch.float64, device=dev)
        self.result = torch.empty(reg.RESULT_DOUBLES, dtype=torch.float64, device=dev)
        self.ws = reg.register_workspace(len(source), len(target), iterations, dev)
        self.fn = reg.register_icp_raw

    def __call__(self):
        self.fn(self.s, self.t, self.md, self.its, True, 0.0, None, self.c, self.d2, self.hist, self.result, workspace=self.ws)


def timed(call, rounds, reps):
    import torch
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(us), min(us), max(us)


def child():
    """What runs under the profiler: CHILD_WARM + CHILD_CALLS calls of 30 iterations."""
    import torch
    source, target, md = sets()
    call = Call(source, target, md, 30)
    for _ in range(CHILD_WARM + CHILD_CALLS):
        call()
        torch.cuda.synchronize()


def per_kernel(trace_dir):
    """{kernel name: (launches per call, median us, min, max)} from a rocprofv3 kernel trace of child()."""
    os.makedirs(trace_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "-o", "register", "--", sys.executable,
           os.path.abspath(__file__), "--child"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    rows = [r for r in csv.DictReader(open(files[0])) if "register_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call = len(rows) // (CHILD_WARM + CHILD_CALLS)
    out = {}
    for r in rows[CHILD_WARM * per_call:]:
        name = r["Kernel_Name"].split("register_")[1].split("(")[0]
        out.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (len(v) // CHILD_CALLS, statistics.median(v), min(v), max(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--trace", default=None, help="directory for a rocprofv3 kernel trace of a child run: per-kernel times")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-hinge", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(out) + "\n")

    if a.child:
        return child()
    import torch
    assert a.rounds >= 10, "a median of at least 10 windows"
    source, target, md = sets()
    say(f"{torch.cuda.get_device_name(0)} on {platform.node()}, torch {torch.__version__}; {len(source)} source x {len(target)} "
        f"target points, max_distance {md}")
    t = {}
    for its in (0, 1, 30):
        call = Call(source, target, md, its)
        t[its] = timed(call, a.rounds, a.reps)
        rec, hist = call.result.cpu().numpy(), call.hist.cpu().numpy()
        say(f"iterations {its}: mgs_register_icp {t[its][0]:.1f} us ({t[its][1]:.1f} .. {t[its][2]:.1f}); executed {int(rec[16])}, "
            f"inliers {int(rec[15])}, fitness {rec[14]:.4f}, rmse {rec[13]:.5f}, scale {rec[12]:.6f}, cell edge {rec[19]:.4f}, "
            f"grid {int(rec[20])} x {int(rec[21])} x {int(rec[22])}" + (f", first rmse {hist[0, 1]:.5f}" if its else ""))
        del call
    iteration = (t[30][0] - t[0][0]) / 30.0
    build = t[0][0] - iteration
    say()
    say("| what | us |")
    say("|---|---|")
    say(f"| grid build (t0 - one iteration) | {build:.1f} |")
    say(f"| one iteration, query + solve ((t30 - t0) / 30) | {iteration:.1f} |")
    say(f"| a 30-iteration call | {t[30][0]:.1f} ({t[30][1]:.1f} .. {t[30][2]:.1f}) |")
    say(f"| per source point and iteration | {1e3 * iteration / len(source):.3f} ns |")
    if not a.skip_hinge:
        from robosimgs_amd import articulation as art
        dev = torch.device("cuda")
        ts, tt = torch.from_numpy(source).to(dev), torch.from_numpy(target).to(dev)
        joint = torch.empty(art.JOINT_DOUBLES, dtype=torch.float64, device=dev)
        ws = art.hinge_workspace(len(source), len(target), dev)
        med, lo, hi = timed(lambda: art.hinge_fit_raw(ts, tt, 0.01, None, None, joint, workspace=ws), 10, 1)
        pairs = 2.0 * len(source) * len(target)
        per_pair = med * 1e-6 / pairs
        say()
        say(f"yardstick: mgs_hinge_fit on the same sets {med / 1e3:.1f} ms ({lo / 1e3:.1f} .. {hi / 1e3:.1f}) for {pairs:.3g} pairs (both "
            f"directions): {per_pair * 1e12:.3f} ps per pair, {med / 2e3:.1f} ms per direction")
        say(f"one grid iteration costs what {iteration * 1e-6 / per_pair:.3g} brute-force pairs cost: {iteration * 1e-6 / per_pair / len(source):.1f} "
            f"per source point, against the {len(target)} a brute-force pass evaluates ({med / 2 / iteration:.0f} x)")
    if a.trace:
        say()
        say("| kernel | launches per call | us (min .. max) |")
        say("|---|---|---|")
        for name, (n, med, lo, hi) in per_kernel(a.trace).items():
            say(f"| register_{name} | {n} | {med:.1f} ({lo:.1f} .. {hi:.1f}) |")


if __name__ == "__main__":
    main()
