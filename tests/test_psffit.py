"""CPU checks of the PSF fit: the numpy restatement
(tests/psffit_ref.py) recovers the model that generated a frame and agrees
with numpy.linalg.lstsq on the explicit design matrix; its model evaluation is
oracle/psf_oracle.py's; PSF.from_values / PSF.write / PSF(path) round-trip
every value exactly; check_fit_args refuses what the device cannot take; the
binding lists both entry points; and the condition the GPU clipping test
rests on (every dropped star at least twice the threshold, every kept star at
most half) holds for its case.

The recovery case's error, recorded here as the yardstick of the GPU tests'
kind of bound: noise-free, known flux and sky, 9 stars, hw = 6 on an 80 x 80
frame: predicted stamps differ from the generating ones by 1.3e-14 of the
peak (lstsq: 8.5e-16).  The assertion allows 1e-12: the scaled normal matrix
has a condition of 1.4e3 to 1.5e4, and 1.5e4 * 2^-53 = 1.7e-12 bounds what
rounding may do to the coefficients, of which the stamps see less."""
import warnings

import numpy as np
import pytest

import psf_oracle
import psffit_ref as R


def test_restatement_recovers_the_truth():
    cfg = R.config(6, 80, 80)
    img, xy, flux, truth = R.make_frame(cfg, 9, 7, sky=R.SKY)
    res = R.fit(cfg, img, xy, flux=flux, sky=R.SKY)
    assert res["frame_status"] == 0 and res["used"].all() and res["rounds"] == 0
    assert (res["status"] == 0).all() and (res["npix"] >= cfg["ncomp"]).all()
    err = R.stamp_error(cfg, res["coef"], truth, xy)
    ls = R.lstsq_fit(cfg, res)
    err_ls = R.stamp_error(cfg, ls, truth, xy)
    agree = R.stamp_error(cfg, res["coef"], ls, xy)
    print(f"restatement vs truth {err:.3g}, lstsq vs truth {err_ls:.3g}, restatement vs lstsq "
          f"{agree:.3g}; largest rms {np.nanmax(res['rms']):.3g}")
    assert err < 1e-12 and err_ls < 1e-12 and agree < 1e-12
    # noise-free data: the residual is the rounding of the cancellation in rss
    assert np.nanmax(res["rms"]) < 1e-6


def test_restatement_evaluates_like_the_oracle():
    cfg = R.config(4, 40, 40)
    coef = R.truth_coeffs(cfg)
    hdr, c = psf_oracle.read_model(R.GOLDEN_PSF)
    np.testing.assert_array_equal(coef, c)
    hdr = dict(hdr, hw=4, x_orig=cfg["origin"][0], y_orig=cfg["origin"][1])
    xy = [(3.25, 30.5), (20.0, 20.0)]
    want = psf_oracle.spatial_stamps(hdr, c, xy, normalize=False)
    got = R.stamps(cfg, coef, xy)
    assert np.max(np.abs(got - want)) <= 4 * np.finfo(float).eps * np.max(np.abs(want))
    # real offsets: one pixel against calc_psf_pix
    loc = psf_oracle.local_coeffs(hdr, c, 3.25, 30.5)
    phi = R.basis(cfg, np.array([0.37]), np.array([-1.61]))
    assert phi[0] @ np.array(loc) == pytest.approx(psf_oracle.calc_psf_pix(hdr, loc, 0.37, -1.61),
                                                    rel=1e-14)


def test_from_values_write_read_round_trip(tmp_path):
    import psf_calculate as pc
    rng = np.random.default_rng(3)
    coef = rng.standard_normal(36) * 10.0 ** rng.integers(-8, 3, size=36)
    vals = dict(hw=7, ngauss=2, ldeg=2, sdeg=1, cos=0.1 + 1 / 3, sin=-np.sqrt(0.5), ax=-1 / 7,
                ay=-0.166165, sigma_inc=0.548, x_orig=225.5, y_orig=1 / 3, coeffs=coef,
                recenter=1.0, sigma_mscale=1.582, fitrad=np.pi)
    m = pc.PSF.from_values(**vals)
    assert m.ncomp == 12 and m.ntot == 36 and m.coeffs == list(coef)
    path = tmp_path / "model.bin.txt"
    m.write(str(path))
    assert len(path.read_text().splitlines()) == 14 + 36
    r = pc.PSF(str(path))
    for k in ("hw", "ndeg_spat", "ndeg_local", "ngauss", "recenter", "cos", "sin", "ax", "ay",
              "sigma_inc", "sigma_mscale", "fitrad", "x_orig", "y_orig", "ldeg", "sdeg", "ntot"):
        assert getattr(r, k) == getattr(m, k), k
        assert type(getattr(r, k)) is type(getattr(m, k)), k
    assert r.vec_coeffs == m.vec_coeffs  # every float64 exactly
    assert (r.hw, r.ndeg_spat, r.ndeg_local, r.fitrad) == (7, 1, 2, np.pi)
    # the golden file survives the same round trip
    g = pc.PSF(R.GOLDEN_PSF)
    g2 = pc.PSF.from_values(g.hw, g.ngauss, g.ldeg, g.sdeg, g.cos, g.sin, g.ax, g.ay, g.sigma_inc,
                            g.x_orig, g.y_orig, g.coeffs, recenter=g.recenter,
                            sigma_mscale=g.sigma_mscale, fitrad=g.fitrad)
    g2.write(str(path))
    g3 = pc.PSF(str(path))
    assert g3.vec_coeffs == g.vec_coeffs and g3.__dict__ == g.__dict__
    # a model of other degrees keeps them, and local_coeffs follows them
    q = pc.PSF.from_values(3, 1, 1, 0, 1.0, 0.0, -0.2, -0.2, 0.5, 10.0, 10.0, [1.0, 2.0, 3.0])
    assert (q.ldeg, q.sdeg, q.ncomp) == (1, 0, 3) and q.local_coeffs(50.0, -3.0) == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="coefficients"):
        pc.PSF.from_values(3, 1, 1, 0, 1.0, 0.0, -0.2, -0.2, 0.5, 10.0, 10.0, [1.0, 2.0])


def test_check_fit_args():
    import psf_calculate as pc
    ok = pc.check_fit_args((80, 80), (9, 2), fwhm=3.0)
    assert ok["ncomp"] == 12 and ok["nterm"] == 3 and ok["origin"] == (40.0, 40.0)
    assert ok["fitrad"] == 15.0 and ok["min_stars"] == 0 and not ok["batched"]
    a = -4.0 * np.log(2.0) / 9.0
    assert ok["shape"] == (1.0, 0.0, a, a) and list(ok["counts"]) == [9]
    b = pc.check_fit_args((5, 80, 80), (5, 16, 2), shape=(1.0, 0.0, -0.1, -0.2), counts=[16, 0, 3, 9, 1],
                          mask_shape=(5, 80, 80), flux_shape=(5, 16), background_shape=(5, 80, 80))
    assert b["batched"] and b["sky_mode"] == 2 and list(b["counts"]) == [16, 0, 3, 9, 1]
    assert pc.check_fit_args((80, 80), (9, 2), fwhm=3.0, background_shape=(9,))["sky_mode"] == 1
    # 3 Gaussians x 6 local x 6 spatial terms is the largest model
    assert pc.check_fit_args((80, 80), (9, 2), fwhm=3.0, ngauss=3, sdeg=2)["ncomp"] == 18

    def bad(match, ishape=(80, 80), pshape=(9, 2), **kw):
        kw.setdefault("fwhm", 3.0)
        with pytest.raises(ValueError, match=match):
            pc.check_fit_args(ishape, pshape, **kw)

    bad("FIT_MAX_COEF", ngauss=4, sdeg=2)           # P = 144 > 108
    bad("FIT_MAX_COEF", ngauss=2, ldeg=3, sdeg=2)   # P = 120
    bad("hw must be", hw=0)
    bad("hw must be", hw=-3)
    bad("hw must be", hw=7.5)                       # 2 hw + 1 = 16: an even box
    bad("hw must be", hw=256)
    bad("fitrad", fitrad=0.0)
    bad("fitrad", fitrad=-2.0)
    bad("fitrad", fitrad=float("nan"))
    bad("exactly one", fwhm=3.0, shape=(1.0, 0.0, -0.1, -0.1))
    bad("exactly one", fwhm=None)
    bad("fwhm", fwhm=0.0)
    bad("shape must be", fwhm=None, shape=(1.0, 0.0, -0.1))
    bad("positions must be", pshape=(9, 3))
    bad("positions must be", pshape=(9,))
    bad("positions must be", pshape=(2, 9, 2))                      # a batch beside one image
    bad("positions must be", ishape=(5, 80, 80), pshape=(4, 9, 2))  # another batch size
    bad("counts must lie", ishape=(2, 80, 80), pshape=(2, 9, 2), counts=[9, 10])
    bad("counts must lie", ishape=(2, 80, 80), pshape=(2, 9, 2), counts=[-1, 3])
    bad("counts must be", ishape=(2, 80, 80), pshape=(2, 9, 2), counts=[1, 2, 3])
    bad("counts goes with", counts=[9])
    bad("FIT_MAX_STARS", pshape=(4097, 2))
    bad("mask shape", mask_shape=(80, 81))
    bad("mask shape", ishape=(2, 80, 80), pshape=(2, 9, 2), mask_shape=(80, 80))
    bad("flux shape", flux_shape=(8,))
    bad("weights shape", weights_shape=(9, 1))
    bad("background shape", background_shape=(3, 3))
    bad("niter", niter=-1)
    bad("nsig", nsig=float("nan"))
    bad("min_stars", min_stars=-1)
    bad("origin", origin=(1.0,))
    bad("image must be", ishape=(80,), pshape=(9, 2))


def test_fit_psf_checks_before_the_device():
    """The checks run on the host, before anything asks for a GPU."""
    import psf_calculate as pc
    img = np.zeros((40, 40))
    with pytest.raises(ValueError, match="exactly one"):
        pc.fit_psf(img, np.zeros((3, 2)))
    with pytest.raises(ValueError, match="positions must be"):
        pc.fit_psf(img, np.zeros((3, 3)), fwhm=3.0)
    with pytest.raises(ValueError, match="mask shape"):
        pc.fit_psf(img, np.zeros((3, 2)), fwhm=3.0, mask=np.zeros((40, 41), dtype=bool))
    x, y = np.array([1.0, 2.0]), np.array([3.0, 4.0])
    np.testing.assert_array_equal(pc._fit_positions((x, y)), [[1.0, 3.0], [2.0, 4.0]])
    np.testing.assert_array_equal(pc._fit_positions({"xcentroid": x, "ycentroid": y}),
                                  [[1.0, 3.0], [2.0, 4.0]])


def test_abi_lists_the_fit():
    import _bsgp
    assert "bsgp_psf_fit_moments" in _bsgp.EXPORTED and "bsgp_psf_fit_solve" in _bsgp.EXPORTED
    L = _bsgp.lib()
    assert L.bsgp_abi_version() == 3
    assert len(L.bsgp_psf_fit_moments.argtypes) == 23 and len(L.bsgp_psf_fit_solve.argtypes) == 20
    # argument validation runs on the host without a device
    m = _bsgp.PsfModel(hw=6, ngauss=4, ldeg=2, sdeg=2, cos=1.0, sin=0.0, ax=-0.1, ay=-0.1,
                       sigma_inc=0.548, x_orig=0.0, y_orig=0.0, coeffs=None, ncoef=0)
    byref = _bsgp.ctypes.byref
    rc = L.bsgp_psf_fit_solve(1, 4, None, None, byref(m), None, None, None, None, None, None, 0, 2.0,
                              0, None, None, None, None, None, None)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and b"144 coefficients" in L.bsgp_last_error()
    m.ngauss = 2
    rc = L.bsgp_psf_fit_solve(1, 4097, None, None, byref(m), None, None, None, None, None, None, 0,
                              2.0, 0, None, None, None, None, None, None)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and b"4097 stars" in L.bsgp_last_error()
    rc = L.bsgp_psf_fit_moments(None, 1, 1, 8, 8, None, None, 4, byref(m), 0.0, None, None, 0, None,
                                0, 0.0, None, None, None, None, None, None, None)
    assert rc == _bsgp.BSGP_ERR_ARG and b"fitrad" in L.bsgp_last_error()
    rc = L.bsgp_psf_fit_moments(None, 1, 0, 8, 8, None, None, 4, byref(m), 3.0, None, None, 0, None,
                                0, 0.0, None, None, None, None, None, None, None)
    assert rc == 0  # B == 0: a no-op that follows no pointer


def test_clipping_case_has_its_margins():
    """The condition of the GPU clipping test (tests/test_gpu_psffit.py, test
    4), checked on the restatement: in every round every dropped star's rms is
    at least twice the threshold and every kept star's at most half, so that
    rounding cannot move a star across; exactly the two contaminated stars go."""
    cfg, args, _, bad = R.clip_case()
    trace = []
    res = R.fit(cfg, trace=trace, **args)
    assert sorted(np.flatnonzero(~res["used"])) == sorted(bad) and res["rounds"] == 1
    assert len(trace) == 2  # the round that drops them, and one that drops nothing
    for thr, rms, drop in trace:
        for s, r in rms.items():
            print(f"thr {thr:.4g} star {s} rms/thr {r / thr:.3f} {'dropped' if s in drop else ''}")
            assert r / thr >= 2.0 if s in drop else r / thr <= 0.5
    assert (res["status"][list(bad)] == R.CLIPPED).all()


def test_restatement_flags():
    """The geometry case's exclusions, as the design states them."""
    cfg, args, _ = R.geometry_case()
    res = R.fit(cfg, **args)
    assert list(res["status"]) == [R.PARTIAL, 0, 0, 0, 0, 0, 0, 0, 0, R.NO_OVERLAP, R.BAD_POSITION]
    assert list(res["used"]) == [True] * 9 + [False] * 2
    full = min(res["npix"][[1, 2, 3, 5, 6, 7]])  # whole boxes, nothing skipped
    assert res["npix"][0] < full and res["npix"][4] < full and res["npix"][8] < full
    assert list(res["npix"][9:]) == [0, 0]
    # weights and fluxes that exclude
    w = np.ones(11)
    w[2], w[3] = 0.0, np.nan
    f = args["flux"].copy()
    f[5] = -1.0
    r2 = R.fit(cfg, **dict(args, flux=f), weights=w)
    assert r2["status"][2] == R.BAD_WEIGHT and r2["status"][3] == R.BAD_WEIGHT
    assert r2["status"][5] == R.BAD_FLUX and r2["used"].sum() == 6
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        two = R.fit(cfg, args["image"], args["xy"][1:3], flux=args["flux"][1:3], sky=R.SKY)
    assert two["frame_status"] == R.SINGULAR and np.isnan(two["coef"]).all()
