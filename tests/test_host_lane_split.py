"""Host-side unit test of the wide row passes' lane and index maps
(csrc/bsgp_lanesplit.hpp; CPU, no GPU): tests/cpp/lane_split_test.cpp
simulates the 64 lanes, the half-wave swap, the loads, the stores and the
reductions of per-lane partial sums."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beta-sgp_amd", "csrc")


def test_lane_split(tmp_path):
    exe = tmp_path / "lane_split_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "lane_split_test.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
