"""What the compiler makes of raster_fwd_kernel<4, false, false> (robosimgs_amd/csrc/raster_fwd.hip), the kernel of the
headline frame: the hand-written blend statement names some seventy operands, and the kernel sits at the edge of five
waves per SIMD.  Taken from the compiler's own resource report (-Rpass-analysis=kernel-resource-usage) with build.py's
flags, the way profiles/raster_shared/README.md reads its table; the instruction stream is not searched.  No GPU needed."""
import re
import subprocess

import pytest

from robosimgs_amd.csrc import build as B

KERNEL = "raster_fwd_kernelILi4ELb0ELb0EE"          # raster_fwd_kernel<4, false, false>


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = tmp_path_factory.mktemp("raster_fwd_asm") / "raster_fwd.s"
    src = "raster_fwd.hip"
    cmd = [B._hipcc(), *B.FLAGS, *B.PER_SOURCE_FLAGS.get(src, []), "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", f"{B.HERE}/{src}", "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return kernels


def test_headline_kernel_resources(report):
    mine = [v for k, v in report.items() if KERNEL in k]
    assert len(mine) == 1, sorted(report)
    r = mine[0]
    print(r)
    assert int(r["VGPRs"]) <= 96                        # five waves per SIMD
    assert int(r["Occupancy [waves/SIMD]"]) >= 5
    assert int(r["ScratchSize [bytes/lane]"]) <= 8      # no more than before the blend became one statement per entry
    assert int(r["SGPRs Spill"]) == 0
    assert int(r["TotalSGPRs"]) <= 102
