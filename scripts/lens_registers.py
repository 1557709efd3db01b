"""Register use of the MGS_CAMERA_FISHEYE_KB instantiations beside their ideal-fisheye twins (profiles/lens/README.md).

Cross-compiles projection.hip and backward.hip for gfx950 with build.py's flags (device only, to assembly; no GPU needed)
and reads VGPR / SGPR / scratch of every kernel from the code object's metadata.  Prints one line per pair of
instantiations that differ in the camera model only:

    python scripts/lens_registers.py [--all]      # default: the SH-degree-3 kernels of the bench scene and the operators
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robosimgs_amd.csrc import build as B  # noqa: E402

# position of the camera model among each kernel's template arguments
CAM_ARG = {"projection_fwd_kernel": 0, "projection_bwd_kernel": 0, "project_color_fwd_kernel": 3, "project_color_bwd_kernel": 4}
ARGS = {"project_color_fwd_kernel": "DEG, STAGED, RULE, CAM", "project_color_bwd_kernel": "DEG, STAGED, ACCUM, VIEWGRAD, CAM, RAW",
        "projection_fwd_kernel": "CAM", "projection_bwd_kernel": "CAM"}


def kernels(src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([B._hipcc(), *B.FLAGS, "--cuda-device-only", "-S", os.path.join(B.HERE, src), "-o", out], check=True)
        text = open(out).read()
    res = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        get = lambda key: int(re.search(key + r":\s+(\d+)", block).group(1))
        res[name] = (get(r"\.vgpr_count"), get(r"\.sgpr_count"), get(r"\.private_segment_fixed_size"), get(r"\.vgpr_spill_count"))
    names = list(res)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    table = {}
    for mangled, d in zip(names, plain):
        m = re.search(r"(\w+)<(.*?)>\(", d)
        if m and m.group(1) in CAM_ARG:
            table[(m.group(1), tuple(a.strip() for a in m.group(2).split(",")))] = res[mangled]
    return table


def main():
    show_all = "--all" in sys.argv
    print("kernel<template arguments>: VGPR / SGPR / scratch bytes / spilled VGPRs -- fisheye_kb | ideal fisheye")
    for src in ("projection.hip", "backward.hip"):
        table = kernels(src)
        for (kernel, args), kb in sorted(table.items()):
            i = CAM_ARG[kernel]
            if args[i] != "3":
                continue
            if not show_all and len(args) > 1 and (args[0] != "3" or args[1] != "true"):
                continue
            twin = table[(kernel, args[:i] + ("2",) + args[i + 1:])]
            print(f"{kernel}<{ARGS[kernel]}> = <{', '.join(args)}>: {' / '.join(map(str, kb))} | {' / '.join(map(str, twin))}")


if __name__ == "__main__":
    main()
