"""Address- and undefined-behaviour-sanitizer run of the mesh rasteriser's index arithmetic on the CPU.

    python scripts/mesh_host_sanitize.py

Builds tests/host_harness/mesh_harness.cpp (csrc/mesh_raster.h walked launch by launch on heap buffers of exactly the ABI's
sizes) with tests/host_harness/mesh_harness_main.cpp into one stand-alone binary, g++ -O1 -g -fsanitize=address,undefined
-fno-sanitize-recover=all, writes the scenes to a temporary file and runs the binary on it: every raster case at 37 x 29
and 64 x 64, the kernel's own threshold boxes, the 2064 x 16 image, the open box from `top` at 1920 x 1080 (also posed, with
two cameras) and the 1920 x 1080 close-up with more than a thousand faces on the large-face path.  A developer tool for a
machine without a GPU: no Python in the sanitized process, not a pytest test, never a GPU job.  Exit status 0 = clean."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_ref as MR          # noqa: E402
import mesh_scenes as MS       # noqa: E402

HARNESS = os.path.join(ROOT, "tests", "host_harness")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe, scenes = os.path.join(tmp, "mesh_sanitize"), os.path.join(tmp, "scenes.bin")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-ffp-contract=off", os.path.join(HARNESS, "mesh_harness.cpp"), os.path.join(HARNESS, "mesh_harness_main.cpp"),
                        "-o", exe], check=True)
        names = []
        with open(scenes, "wb") as fh:
            for W, H in ((37, 29), (64, 64)):
                for name, c in MR.raster_cases(W, H).items():
                    col = np.random.default_rng(5).uniform(size=(len(c["verts"]), 3))
                    MS.write_scene(fh, c["verts"], c["faces"], MS.IDENTITY_VIEW, c["K"][None], W, H, near=c["near"], far=c["far"],
                                   cull=c["cull"], vertex_colors=col, headlight=True)
                    names.append(f"{name} {W}x{H}")
            c = MS.own_threshold_case()
            MS.write_scene(fh, c["verts"], c["faces"], MS.IDENTITY_VIEW, c["K"][None], 64, 64)
            names.append("own threshold boxes 64x64")
            c = MS.wide_case()
            MS.write_scene(fh, c["verts"], c["faces"], MS.IDENTITY_VIEW, c["K"][None], c["width"], c["height"])
            names.append("wide 2064x16")
            box = MS.openbox()
            vm, K = MS.top_1080p(box)
            MS.write_scene(fh, box["verts"], box["faces"], vm[None], K[None], 1920, 1080, headlight=True)
            names.append("open box, top, 1920x1080")
            R, t = MS.lid_pose(0.6)
            vm2, K2 = MS.closeup_1080p(box)
            MS.write_scene(fh, box["verts"], box["faces"], np.stack([vm, vm2]), np.stack([K, K2]), 1920, 1080, link_ids=box["link_ids"],
                           rotations=R, translations=t, face_colors=np.random.default_rng(6).uniform(size=(len(box["faces"]), 3)))
            names.append("open box posed, top + close-up, 2 cameras, 1920x1080")
            MS.write_scene(fh, box["verts"], box["faces"], vm2[None], K2[None], 1920, 1080, headlight=True)
            names.append("open box, close-up, 1920x1080")
        r = subprocess.run([exe, scenes], capture_output=True, text=True)
        lines = r.stdout.splitlines()
        for line, name in zip(lines, names):
            print(f"{line}   [{name}]")
        for line in lines[len(names):]:
            print(line)
        if r.returncode != 0 or r.stderr.strip():
            print(r.stderr[-6000:], file=sys.stderr)
            print(f"FAILED: exit status {r.returncode}", file=sys.stderr)
            return 1
        closeup = lines[len(names) - 1]
        listed = int(closeup.split("faces,")[1].split("on the")[0])
        assert listed >= 1000, f"the close-up has only {listed} faces on the large-face path"
    return 0


if __name__ == "__main__":
    sys.exit(main())
