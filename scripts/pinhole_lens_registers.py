"""Register use of the MGS_CAMERA_PINHOLE_BC instantiations beside their plain-pinhole twins
(profiles/pinhole_lens/README.md).

scripts/lens_registers.py's cross-compile of projection.hip and backward.hip for gfx950 (device only, to assembly; no GPU
needed), read for the fifth camera model: one line per pair of instantiations that differ in the camera model only.

    python scripts/pinhole_lens_registers.py [--all]      # default: the SH-degree-3 staged kernels and the operators
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lens_registers import ARGS, CAM_ARG, kernels  # noqa: E402

LENS, TWIN = "4", "0"      # MGS_CAMERA_PINHOLE_BC, MGS_CAMERA_PINHOLE


def main():
    show_all = "--all" in sys.argv
    print("kernel<template arguments>: VGPR / SGPR / scratch bytes / spilled VGPRs -- pinhole_bc | plain pinhole")
    worst = [0, 0]
    for src in ("projection.hip", "backward.hip"):
        table = kernels(src)
        for (kernel, args), lens in sorted(table.items()):
            i = CAM_ARG[kernel]
            if args[i] != LENS:
                continue
            worst = [max(worst[0], lens[2]), max(worst[1], lens[3])]
            if not show_all and len(args) > 1 and (args[0] != "3" or args[1] != "true"):
                continue
            twin = table[(kernel, args[:i] + (TWIN,) + args[i + 1:])]
            print(f"{kernel}<{ARGS[kernel]}> = <{', '.join(args)}>: {' / '.join(map(str, lens))} | {' / '.join(map(str, twin))}")
    print(f"over every pinhole_bc instantiation: largest scratch {worst[0]} bytes, most spilled VGPRs {worst[1]}")


if __name__ == "__main__":
    main()
