"""Star-stamp metrics, the part that needs no GPU: the fixture
against its numpy / scipy statement, the host build of the lmder port against
the fixture, the argument checks, the exported symbols."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
from stamps_ref import check_fit, same_bits


@pytest.fixture(scope="module")
def fx():
    return golden("stampmetrics_cases.npz")


def test_fixture_agrees_with_its_statement(fx):
    pytest.importorskip("scipy")
    import stamps_ref as R
    for i in range(48):
        p = R.radial_profile(fx["stamps"][i], fx["stamp_center"][i])
        assert len(p) == fx["stamp_len"][i] and same_bits(p, fx["stamp_prof"][i, :len(p)])
        assert same_bits(fx["fit_prof"][i], fx["stamp_prof"][i])
    for name in fx["pc_names"]:
        p = R.radial_profile(fx[f"pc_img_{name}"].astype(np.float64), fx[f"pc_center_{name}"])
        assert same_bits(p, fx[f"pc_prof_{name}"]), name
    assert np.sum(fx["fit_ier"] == 5) >= 3
    assert np.all(fx["fit_resp"] < 1e-10) and np.all(fx["fit_resp_perr"] < 1e-10)
    for i in range(len(fx["fit_len"])):
        f = R.fit_gauss1d(fx["fit_prof"][i, :fx["fit_len"][i]], fx["fit_fwhm"][i])
        check_fit(fx, i, f["fitted"], f["perr"], f["ier"], f["nfev"])
    from scipy.stats import wasserstein_distance
    for k in range(len(fx["w1_d"])):
        u, v = fx["w1_u"][k, :fx["w1_ulen"][k]], fx["w1_v"][k, :fx["w1_vlen"][k]]
        d, dabs = R.wasserstein1(u, v)
        assert same_bits(d, fx["w1_d"][k]) and same_bits(dabs, fx["w1_abs"][k])
        if np.isfinite(d):
            assert d == wasserstein_distance(u, v)
    assert fx["w1_d"][list(fx["w1_names"]).index("equal")] == 0.0


def test_host_build_of_the_lmder_port_meets_the_fixture(fx, tmp_path):
    """csrc/bsgp_lmder.hpp with a team of one lane (tests/cpp/lmder_host.cpp):
    the same ier and nfev as scipy's leastsq on every fit, the maxfev ones
    included, and fitted / perr within the bars the device build must meet."""
    # g++ as build() uses it for the host unit test, else the ROCm clang++ that
    # hipcc itself runs; with neither the test fails: nothing else on the CPU
    # checks the port
    cxx = shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    so = str(tmp_path / "liblmder_host.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                    os.path.join(ROOT, "beta-sgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "lmder_host.cpp"), "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.lmder_host_fit.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, vp, vp, vp, vp]
    L.lmder_host_fit.restype = None
    rcap = fx["fit_prof"].shape[1]

    def fit(prof, n, fwhm):
        prof = np.ascontiguousarray(prof, np.float64)
        fitted, par, perr = np.zeros(rcap), np.zeros(3), np.zeros(3)
        info = np.zeros(2, np.int32)
        L.lmder_host_fit(prof.ctypes.data, n, rcap, float(fwhm), fitted.ctypes.data,
                         par.ctypes.data, perr.ctypes.data, info.ctypes.data)
        return fitted, par, perr, info

    worst = 0.0
    for i in range(len(fx["fit_len"])):
        fitted, par, perr, info = fit(fx["fit_prof"][i], int(fx["fit_len"][i]), fx["fit_fwhm"][i])
        worst = max(worst, check_fit(fx, i, fitted, perr, info[0], info[1]))
        assert np.all(np.isnan(fitted[fx["fit_len"][i]:]))
    print(f"host lmder port: largest difference {worst:.3g} of its bar")
    # the documented flags
    fitted, par, perr, info = fit(np.zeros(rcap), 2, 3.0)
    assert tuple(info) == (0, 0) and np.all(np.isnan(fitted)) and np.all(np.isnan(par))
    bad = np.ones(rcap)
    bad[4] = np.inf
    fitted, par, perr, info = fit(bad, 9, 3.0)
    assert tuple(info) == (0, 0) and np.all(np.isnan(perr))
    fitted, par, perr, info = fit(np.zeros(rcap), 9, 3.0)
    assert tuple(info) == (int(fx["sing_ier"]), int(fx["sing_nfev"]))
    assert np.all(np.isnan(perr)) and same_bits(fitted[:9], fx["sing_fitted"])
    # the narrow starts went through trial points with non-finite residuals
    assert np.sum(fx["fit_nonfinite_trials"] > 0) >= 3


def test_argument_checks_need_no_gpu():
    import stamps as S
    ok = np.zeros((5, 9))
    for shape, c in [((4,), (0, 0)), ((0, 3), (0, 0)), ((2, 3, 4, 5), (0, 0)),
                     ((129, 128), (0, 0)),                    # more than 16384 pixels
                     ((5, 9), (0.0, np.nan)), ((5, 9), (np.inf, 1.0)), ((5, 9), (1.0,)),
                     ((3, 5, 9), np.zeros((2, 2))),
                     ((1, 300), (0.0, 0.0)),                  # 300 bins
                     ((1, 257), (0.0, 0.0)), ((5, 9), (1e300, 0.0))]:
        with pytest.raises(ValueError):
            S.check_profile_args(shape, np.asarray(c))
    assert S.check_profile_args((1, 256), np.zeros(2))[2] == 256
    assert S.check_profile_args((3, 5, 9), (1.3, 6.6))[2] == 8  # int(sqrt(2.7^2 + 6.6^2)) + 1
    with pytest.raises(ValueError):
        S.radial_profile(np.zeros((1, 300)), (0.0, 0.0))
    for f in (0.0, -1.0, np.nan, np.inf, [1.0, 2.0]):
        with pytest.raises(ValueError):
            S.fit_radprof(np.ones(9), f)
    with pytest.raises(ValueError):
        S.fit_radprof(np.ones((2, 3, 4)), 2.0)
    with pytest.raises(ValueError):
        S.fit_radprof(np.ones(257), 2.0)
    with pytest.raises(ValueError):
        S.fit_radprof(np.ones((2, 9)), 2.0, lengths=[9])
    with pytest.raises(ValueError):
        S.wasserstein_distance_norm(np.ones(300), np.ones(3))
    with pytest.raises(ValueError):
        S.wasserstein_distance_norm(np.ones((2, 5)), np.ones(5))
    with pytest.raises(ValueError):
        S.wasserstein_distance_norm(np.ones((2, 5)), np.ones((3, 5)))
    with pytest.raises(ValueError):
        S.stamp_metrics(ok, ok[None], (0, 0), (0, 0), 2.0, 2.0)
    with pytest.raises(ValueError):
        S.stamp_metrics(ok[None], ok[None], (0, 0), (0, 0), 2.0, -2.0)
    # the table form of the reference's call: element 0 of the 'fwhm' column
    assert float(S._fwhm_of({"fwhm": np.array([3.5, 9.0])})) == 3.5


def test_entry_points_exported_and_validate_on_the_host():
    import _bsgp
    L = _bsgp.lib()
    for name in ("bsgp_radial_profile", "bsgp_fit_gauss1d", "bsgp_wasserstein1"):
        assert name in _bsgp.EXPORTED and hasattr(L, name)
    assert L.bsgp_abi_version() == 3
    buf = np.zeros(64)
    p = ctypes.c_void_p(buf.ctypes.data)  # never dereferenced: every call below fails validation

    def prof(data=p, dtype=1, B=1, H=8, W=8, centers=p, rcap=12, out=p, length=p):
        rc = L.bsgp_radial_profile(data, dtype, B, H, W, centers, rcap, out, length, None)
        return rc, L.bsgp_last_error()

    assert prof(data=None)[0] == _bsgp.BSGP_ERR_ARG
    assert prof(centers=None)[0] == _bsgp.BSGP_ERR_ARG
    assert prof(dtype=7)[0] == _bsgp.BSGP_ERR_ARG
    assert prof(rcap=0)[0] == _bsgp.BSGP_ERR_ARG
    rc, msg = prof(H=129, W=128)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and b"16384" in msg
    rc, msg = prof(rcap=257)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and b"256" in msg
    assert L.bsgp_fit_gauss1d(p, None, 1, 8, p, p, p, p, p, None) == _bsgp.BSGP_ERR_ARG
    assert L.bsgp_fit_gauss1d(p, p, 1, 257, p, p, p, p, p, None) == _bsgp.BSGP_ERR_UNSUPPORTED
    assert L.bsgp_wasserstein1(None, p, p, p, 1, 8, p, None) == _bsgp.BSGP_ERR_ARG
    assert L.bsgp_wasserstein1(p, p, p, p, 1, 257, p, None) == _bsgp.BSGP_ERR_UNSUPPORTED
