"""The penalty-shape table of the register kernels (csrc/wfa_shapes.hpp) and what the launchers decide from it, on the host alone:
tools/shape_table_check.cpp includes the kernel headers' host side with stand-ins for the run-time compiler and checks

* the normalisation (x, o + e, e [, o2 + e2, e2]) / gcd and the look-up: 4/6/2, 2/3/1 and 8/12/4 are one shape (index 0), each preset
  has its index, 5/6/2 has none, the gap-affine-2p default has its entry, and the shapes only the lane and segmented kernels are built
  for report no banded / slim unit;
* the names of the run-time instantiations of the lane, segmented, banded and slim kernels, byte for byte (code objects cached on disk
  are keyed on them);
* the route of a banded launch (built-in banded / slim unit, run-time slim or banded kernel) and the kernel form, over every
  combination of chunk count, scope, heuristic, staging, history form and windowing for built-in and run-time shapes of both distance
  functions, with and without hipRTC — against a second, independent statement of the rules; and that what the host tells the walk
  (slim_launches) is "the route is slim".

No GPU and no device code: the program is compiled for the host only."""
import os
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("shape_table") / "shape_table_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-x", "hip", "--cuda-host-only", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "pywfa_amd", "csrc"),
                    os.path.join(ROOT, "tools", "shape_table_check.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe), "--dump"], capture_output=True, text=True)


def test_every_check_passes(report):
    failed = [ln for ln in report.stdout.splitlines() if ln.startswith("FAILED")]
    assert report.returncode == 0 and not failed, "\n".join(failed[:20])
    assert report.stdout.splitlines()[-1].endswith(", 0 failed")


def test_names_cover_every_family_and_form(report):
    names = [ln[5:] for ln in report.stdout.splitlines() if ln.startswith("name ")]
    for want in ("wfa::wfa_lane_kernel<5, 8, 2, false, false>", "wfa::wfa_lane_kernel<5, 8, 2, true, false>",
                 "wfa::wfa_lane_kernel<5, 8, 2, false, true, 0, 16>", "wfa::wfa_seg_kernel<5, 8, 2, 16, true, false, false>"):
        assert want in names
    for family in ("wfa::wfa_band_kernel<", "wfa::wfa_band_kernel_w3<", "wfa::wfa_band_kernel_w4<", "wfa::wfa_slim_kernel<2, ",
                   "wfa::wfa_slim_kernel_tail<4, ", "wfa::wfa_slim_kernel_2p<3, "):
        assert any(n.startswith(family) for n in names), family
    assert any(n.startswith("wfa::wfa_slim_kernel_tail<4, ") and n.endswith(", true>") for n in names)   # the windowed form


def test_every_route_is_reached(report):
    """The grid is only a check if it reaches every kind of route, each built-in unit's shape family, and both answers of slim_launches."""
    rows = [ln for ln in report.stdout.splitlines() if ln.startswith("route ")]
    assert len(rows) == 3 * 5 * 4 * 128 * 3 * 2
    kinds = {ln.split("-> kind ")[1].split()[0] for ln in rows}
    assert kinds == {"0", "1", "2", "3"}
    assert {ln.split(" unit ")[1].split()[0] for ln in rows} == {"-1", "0", "4"}
    assert {ln.rsplit(" ", 1)[1] for ln in rows} == {"0", "1"}
