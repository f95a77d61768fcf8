"""Host-side unit test of the PSF fit's host-compilable pieces (CPU, no GPU):
tests/cpp/psffit_test.cpp holds the packed Cholesky, the triangular solves,
the residual from the moments, the clipping rule and the shared basis of
csrc/bsgp_psffit.hpp / bsgp_psf.hpp against hand-checked matrices.  Built
with g++ as tests/test_host_cpp.py builds its programs, and once more with
-fsanitize=address,undefined where the sanitizer runtimes link: a stand-alone
program on the CPU, nothing of it is loaded into python or touches a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beta-sgp_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "psffit_test.cpp")
# -ffp-contract=off: the same rounding as the gfx950 build
BASE = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC]


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout


def test_psffit_host_cpp(tmp_path):
    exe = tmp_path / "psffit_test"
    subprocess.run(BASE + [SRC, "-o", str(exe)], check=True)
    _run(exe)


def _sanitizers_link(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o",
                        str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0


def test_psffit_host_cpp_sanitized(tmp_path):
    if not _sanitizers_link(tmp_path):
        pytest.skip("the address / undefined-behaviour sanitizer runtimes do not link here")
    exe = tmp_path / "psffit_test_san"
    subprocess.run(BASE + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                           "-o", str(exe)], check=True)
    _run(exe)
