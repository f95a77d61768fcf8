"""Background estimator, the checks that need no device: the golden generator's
self-checks as recorded in tests/golden/bkg2d_cases.npz
(tests/golden/make_golden_bkg.py), the numpy restatement of the spline stage
against scipy's maps, and the argument errors of background.Background2D and
bsgp_background2d, which are raised before any device work."""
import ctypes
import inspect

import numpy as np
import pytest

import bkg_ref

RAW = ("c1raw", "c2raw", "c3raw", "c4raw")
FULL = ("c1", "c2a", "c2b", "c3", "c4", "c5i0", "c5i1", "c5i2")


@pytest.fixture(scope="module")
def fx():
    return bkg_ref.cases()


def test_golden_membership_margin(fx):
    """No pixel of any box lies within 1e-9 of a clipping bound in any
    iteration (the generator refuses to write the file otherwise): a 1e-12
    difference in a standard deviation cannot change the survivors."""
    for tag in RAW + FULL:
        assert float(fx[f"{tag}_margin"]) >= 1e-9, tag
    assert float(fx["c2a_margin"]) > 4e-6  # the application tile, measured 4.5e-6


def test_golden_cases_exercise_what_they_claim(fx):
    assert fx["c1raw_niter"].max() >= 3          # pixels removed in more than one iteration
    assert fx["c1_bkg_mesh"].shape == (7, 7)
    for tag in ("c2raw", "c2a", "c2b"):          # the 10-iteration cap is reached
        assert fx[f"{tag}_niter"].max() == 10, tag
    ex = fx["c2a_excl"]
    assert ex.shape == (7, 7) and ex[-1].all() and ex[:, -1].all() and ex.sum() == 13
    assert not fx["c2b_excl"].any()
    for tag in ("c2a", "c2b"):                   # the clamp is live
        lo, hi = fx[f"{tag}_bkg_unclipped_range"]
        m = fx[f"{tag}_bkg_mesh"]
        assert lo < m.min() or hi > m.max(), tag
    assert fx["c3_nsurv"][0, 0] == 49 and fx["c3_raw_std"][0, 0] == 0 and fx["c3_raw_med"][0, 0] == 42.5
    assert fx["c3_excl"].sum() == 1 and fx["c3_excl"][1, 1]
    assert fx["c3_nanmask"][:7, 14:].sum() == 5 and fx["c3_nanmask"].sum() == 5
    assert fx["c4_bkg_mesh"].shape == (1, 2) and fx["c4_data"].shape == (64, 128)


def test_spline_restatement_matches_scipy_maps(fx):
    """bkg_ref.zoom (the recursion and taps the kernels implement) against the
    golden maps, which are scipy.ndimage.zoom(order=3, mode='reflect',
    grid_mode=True) of the same filtered meshes: rounding apart, on every mesh
    size of the fixture (7x7, 3x3, 1x2)."""
    idx = fx["c2_idx"]
    for tag, box, shape in (("c1", (7, 8), (49, 56)), ("c2a", (60, 60), (375, 375)),
                            ("c2b", (60, 60), (375, 375)), ("c3", (7, 7), (21, 21)),
                            ("c4", (64, 64), (64, 128))):
        for nm in ("bkg", "rms"):
            mesh = fx[f"{tag}_{nm}_mesh"]
            got = bkg_ref.zoom(mesh, box, shape)
            if tag.startswith("c2"):
                got = got[np.ix_(idx, idx)]
            err = np.max(np.abs(got - fx[f"{tag}_{nm}"])) / np.max(np.abs(mesh))
            assert err < 1e-13, (tag, nm, err)
    assert np.all(bkg_ref.zoom(fx["c4_bkg_mesh"], (64, 64), (64, 128))[1:] ==
                  bkg_ref.zoom(fx["c4_bkg_mesh"], (64, 64), (64, 128))[0])


def test_argument_errors_need_no_device():
    from background import Background2D, check_args
    img = np.ones((21, 21))
    for bad in ((2, 3), 4, (3, 0), (3, -1)):
        with pytest.raises(ValueError, match="filter_size"):
            Background2D(img, 7, filter_size=bad)
    for bad in (0, -7, (7, 0)):
        with pytest.raises(ValueError, match="box_size"):
            Background2D(img, bad)
    with pytest.raises(ValueError, match="box_size"):
        Background2D(img, (7, 7, 7))
    with pytest.raises(ValueError, match="mask shape"):
        Background2D(img, 7, mask=np.zeros((21, 20), bool))
    with pytest.raises(ValueError, match="mask shape"):
        Background2D(np.ones((2, 21, 21)), 7, mask=np.zeros((3, 21, 21), bool))
    with pytest.raises(ValueError, match="exclude_percentile"):
        Background2D(img, 7, exclude_percentile=101)
    with pytest.raises(ValueError, match="maxiters"):
        Background2D(img, 7, maxiters=-1)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        Background2D(np.ones(21), 7)
    assert check_args((2, 21, 21), 7, 3, 3.0, 10, 10.0, (21, 21)) == ((7, 7), (3, 3))
    s = inspect.signature(Background2D.__init__)
    assert list(s.parameters)[1:] == ["data", "box_size", "filter_size", "sigma", "maxiters",
                                      "exclude_percentile", "clip", "mask", "device_out"]
    assert s.parameters["filter_size"].default == (3, 3) and s.parameters["sigma"].default == 3.0
    assert s.parameters["maxiters"].default == 10
    assert s.parameters["exclude_percentile"].default == 10.0


def test_no_cpu_fallback():
    import _bsgp
    from background import Background2D
    if _bsgp.torch is not None and _bsgp.torch.cuda.is_available():
        return  # tests/test_gpu_background.py runs it
    with pytest.raises(_bsgp.BsgpError):
        Background2D(np.ones((21, 21)), 7)


def test_c_abi_argument_errors():
    """bsgp_background2d validates on the host before any device call:
    BSGP_ERR_ARG names the field, the box cap is BSGP_ERR_UNSUPPORTED and names
    the limit."""
    import _bsgp
    L = _bsgp.lib()
    assert "bsgp_background2d" in _bsgp.EXPORTED and L.bsgp_abi_version() == 3
    buf = np.zeros((64, 64))
    p = ctypes.c_void_p(buf.ctypes.data)  # never dereferenced: every call below fails validation

    def call(data=p, dtype=1, B=1, H=64, W=64, bh=8, bw=8, fh=3, fw=3, sigma=3.0, maxiters=10,
             excl=10.0):
        rc = L.bsgp_background2d(data, dtype, B, H, W, bh, bw, fh, fw, sigma, maxiters, excl, 1,
                                 None, None, None, None, None, None, None, None)
        return rc, L.bsgp_last_error().decode()

    for kw, word in ((dict(data=None), "data"), (dict(dtype=2), "dtype"), (dict(B=0), "B"),
                     (dict(bh=0), "box size"), (dict(bw=-1), "box size"),
                     (dict(fh=2), "filter size"), (dict(fw=0), "filter size"),
                     (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"),
                     (dict(maxiters=-1), "maxiters"), (dict(excl=100.5), "exclude_percentile")):
        rc, msg = call(**kw)
        assert rc == _bsgp.BSGP_ERR_ARG and word in msg, (kw, rc, msg)
    rc, msg = call(H=65, W=64, bh=65, bw=64)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and "4096" in msg and "4160" in msg, (rc, msg)
    rc, msg = call(fh=9)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and "7 x 7" in msg, (rc, msg)
    rc, msg = call(H=1024, W=1024, bh=8, bw=8)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and "mesh" in msg, (rc, msg)


def test_subdivisions_accept_estimate_keyword():
    import subdivisions
    for fn in (subdivisions.sgp_subdivisions, subdivisions.sgp_subdivisions_multistart):
        s = inspect.signature(fn)
        assert s.parameters["bkg_box_size"].default is None
        assert s.parameters["bkg_filter_size"].default == (3, 3)
        assert list(s.parameters)[:3] == ["image", "psf", "bkg"]
        with pytest.raises(ValueError, match="estimate"):
            fn(np.ones((32, 32)), np.ones((3, 3)) / 9, "median")
        with pytest.raises(ValueError, match="bkg_box_size"):
            fn(np.ones((32, 32)), np.ones((3, 3)) / 9, "estimate")
    assert list(inspect.signature(subdivisions.sgp_subdivisions).parameters)[3:7] == \
        ["subdiv_shape", "overlap", "betaParams", "device_out"]
