"""Resource facts of the plain score-only lane kernel after the probe rework (wfa_lane.hpp): k_lane.hip is compiled to gfx950
assembly with the command line of tools/lane_mix.py, and for the shapes 2/4/1 and 4/7/1 in both widths the kernel must use no
scratch and stay within the registers its occupancy stands on: the 8-diagonal form within what `lane_narrow_waves` asks for (2/4/1:
6 waves per SIMD, at most 80 VGPRs; 4/7/1: 5 waves, at most 96), the 16-diagonal form at 4 waves (at most 128).  No instruction
counts: those are in DESIGN §3.1."""
import os
import re
import shutil
import subprocess

import pytest

import lane_mix

HIPCC = "/opt/rocm/bin/hipcc"
# index of the shape in affine_shapes (csrc/wfa_shapes.hpp) -> (X, OE, E) in units of g
SHAPES = {0: (2, 4, 1), 2: (4, 7, 1)}
# VGPRs a wave may use for that many waves per SIMD (512 registers per lane and SIMD, allocated in blocks of 8)
VGPR_LIMIT = {6: 80, 5: 96, 4: 128}


def narrow_waves(x, oe, e):
    """lane_narrow_waves of wfa_lane.hpp: the waves the rings of the 8-diagonal form allow."""
    r = max(x, oe) + 2 * e + 2
    return 7 if r <= 6 else 6 if r <= 8 else 5 if r <= 11 else 4


def compile_unit(index, out):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(lane_mix.ROOT, "include"), "-I" + lane_mix.CSRC,
           "-DWFA_TU_INDEX=%d" % index, "-DWFA_LANE_REGION_MARKS=1", "--cuda-device-only", "-S", os.path.join(lane_mix.CSRC, "k_lane.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)


def kernel_resources(path, symbol):
    """.vgpr_count and .private_segment_fixed_size of a kernel from the metadata of the assembly."""
    text = open(path).read()
    for block in text.split("  - .agpr_count:")[1:]:
        if re.search(r"\.name:\s+" + re.escape(symbol) + r"\s", block):
            return (int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)),
                    int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    raise AssertionError("no metadata for " + symbol)


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc is not installed: nothing to compile with")
@pytest.mark.parametrize("index", sorted(SHAPES))
def test_probe_rework_keeps_registers_and_no_scratch(tmp_path, index):
    x, oe, e = SHAPES[index]
    out = str(tmp_path / "k_lane.s")
    compile_unit(index, out)
    for nrp, waves in ((4, narrow_waves(x, oe, e)), (8, 4)):
        symbol = "_ZN3wfa15wfa_lane_kernelILi%dELi%dELi%dELb0ELb0ELi0ELi%dEEEvNS_8FastArgsEii" % (x, oe, e, nrp)
        vgprs, scratch = kernel_resources(out, symbol)
        print(f"shape {x}/{oe}/{e}, {2 * nrp} diagonals: {vgprs} VGPRs, {scratch} bytes of scratch; limit {VGPR_LIMIT[waves]} ({waves} waves)")
        assert scratch == 0
        assert vgprs <= VGPR_LIMIT[waves]
