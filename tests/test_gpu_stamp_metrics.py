"""Star-stamp metrics on the device against the fixture
tests/golden/stampmetrics_cases.npz (made by make_golden_stampmetrics.py from
tests/stamps_ref.py: numpy, scipy.optimize.leastsq, scipy.stats).

Bars.  Profiles: bit-equal (the bin sums are added in numpy.bincount's order).
Fits: ier and nfev equal on every case; the fitted profile within
``256 * response_i + 64 * 2**-53`` of the fixture's, relative to max |fitted|,
and perr likewise with its own response.  response_i is the largest change a
4-ulp perturbation of the profile makes (recorded by the generator, below
1e-10 for every case); the factor 256 covers the device's exp (a couple of
ulp) and the butterfly order of the norms (about ten additions per sum), each
over at most 100 evaluations.  Every bar is below 1e-9, more than four orders
under the 4e-5 by which another Levenberg-Marquardt variant differs.
The fits include stamp profiles started from a FWHM of 0.07 pixels, whose first
steps overshoot to trial points with non-finite residuals: lmder rejects those
(actred stays -1) and shrinks delta, and so must the port.
Wasserstein: ``(n + m) * 2**-53 * sum |terms|`` (two summation orders of n + m
terms).
"""
import numpy as np
import pytest

from conftest import golden
from stamps_ref import check_fit, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return golden("stampmetrics_cases.npz")


@pytest.fixture(scope="module")
def S():
    import stamps
    return stamps


@pytest.fixture(scope="module")
def batch48(fx, S):
    """The 48 stamps in one call: (profiles, lengths)."""
    return S.radial_profile(fx["stamps"], fx["stamp_center"])


def test_profiles_of_the_48_stamps_bit_equal(fx, batch48):
    prof, length = batch48
    np.testing.assert_array_equal(length, fx["stamp_len"])
    R = prof.shape[1]
    assert R == fx["stamp_len"].max()
    assert same_bits(prof, fx["stamp_prof"][:, :R])


def test_an_image_alone_gets_its_batch_bits(fx, S, batch48):
    prof, length = batch48
    for i in (0, 7, 8, 47):
        alone = S.radial_profile(fx["stamps"][i], fx["stamp_center"][i])
        assert isinstance(alone, list) and len(alone) == length[i]
        assert same_bits(alone, prof[i, :length[i]])


@pytest.mark.parametrize("name", ["1x1", "1x7", "7x1", "5x9_offcentre", "corner", "outside",
                                  "1x3_empty_bin0", "33x64", "128x128"])
def test_profile_edge_cases_bit_equal(fx, S, name):
    img32, c, ref = fx[f"pc_img_{name}"], fx[f"pc_center_{name}"], fx[f"pc_prof_{name}"]
    wide = S.radial_profile(img32.astype(np.float64), c)
    assert same_bits(wide, ref), name
    # float32 input: the result of its widening
    assert same_bits(S.radial_profile(img32, c), ref), name
    if name == "1x3_empty_bin0":
        assert np.isnan(wide[0]) and len(wide) == 3 and not np.isnan(wide[1])
    if name == "5x9_offcentre":  # rows and columns swapped is another profile
        assert not same_bits(S.radial_profile(img32, c[::-1]), ref)


def test_profile_limits_refused(S):
    with pytest.raises(ValueError, match="256 bins"):
        S.radial_profile(np.ones((1, 300)), (0.0, 0.0))
    with pytest.raises(ValueError, match="16384"):
        S.radial_profile(np.ones((129, 128)), (0.0, 0.0))
    # 256 bins exactly are served
    p = S.radial_profile(np.arange(256.0)[None], (0.0, 0.0))
    assert p == list(np.arange(256.0))


def test_fits_follow_lmder(fx, S):
    import stamps_ref as R
    n = len(fx["fit_len"])
    fitted, perr, params, ier, nfev = S.fit_radprof(fx["fit_prof"], fx["fit_fwhm"],
                                                    lengths=fx["fit_len"], full=True)
    worst = 0.0
    for i in range(n):
        worst = max(worst, check_fit(fx, i, fitted[i], perr[i], ier[i], nfev[i]))
        assert np.all(np.isnan(fitted[i, fx["fit_len"][i]:]))
        # fitted is the model at the returned parameters (the device's exp)
        m = int(fx["fit_len"][i])
        want = R.model(params[i], np.arange(m, dtype=np.float64))
        np.testing.assert_allclose(fitted[i, :m], want, rtol=1e-12, atol=1e-13 * np.max(np.abs(want)))
    assert np.sum(ier == 5) >= 3 and np.all(nfev[ier == 5] == 100)
    narrow = fx["fit_nonfinite_trials"] > 0
    assert np.sum(narrow) >= 3 and np.all(np.isfinite(params[narrow])) and np.all(nfev[narrow] < 10)
    print(f"device fits: largest difference {worst:.3g} of its bar")
    # one profile alone: the reference's call, a list and a table
    i = 3
    alone = S.fit_radprof(list(fx["fit_prof"][i, :fx["fit_len"][i]]),
                          {"fwhm": fx["fit_fwhm"][i:i + 2]}, full=True)
    assert same_bits(alone[0], fitted[i, :fx["fit_len"][i]]) and same_bits(alone[1], perr[i])
    assert (alone[3], alone[4]) == (ier[i], nfev[i])


def test_fit_flags(fx, S):
    prof = np.zeros((4, 9))
    prof[0, :2] = [3.0, 1.0]                        # len 2
    prof[1] = np.exp(-0.5 * np.arange(9.0) ** 2 / 4.0)
    prof[1, 5] = np.nan                             # a NaN inside the length
    prof[2] = 0.0                                   # singular R
    prof[3] = prof[1]
    prof[3, 5] = np.inf
    fitted, perr, params, ier, nfev = S.fit_radprof(prof, 3.0, lengths=[2, 9, 9, 9], full=True)
    for i in (0, 1, 3):
        assert (ier[i], nfev[i]) == (0, 0)
        assert np.all(np.isnan(fitted[i])) and np.all(np.isnan(perr[i])) and np.all(np.isnan(params[i]))
    assert (ier[2], nfev[2]) == (int(fx["sing_ier"]), int(fx["sing_nfev"]))
    assert np.all(np.isnan(perr[2])) and same_bits(fitted[2], fx["sing_fitted"])
    assert same_bits(params[2], fx["sing_params"])
    # three values: a fit, but no degrees of freedom for the errors
    i = int(np.nonzero(fx["fit_len"] == 3)[0][0])
    f3 = S.fit_radprof(fx["fit_prof"][i, :3], fx["fit_fwhm"][i], full=True)
    assert f3[3] == fx["fit_ier"][i] and np.all(np.isnan(f3[1]))


def test_wasserstein(fx, S):
    d = S.wasserstein_distance_norm(fx["w1_u"], fx["w1_v"], fx["w1_ulen"], fx["w1_vlen"])
    names = list(fx["w1_names"])
    for k, name in enumerate(names):
        ref = fx["w1_d"][k]
        if np.isnan(ref):
            assert name in ("nan", "inf") and np.isnan(d[k])
            continue
        bar = (int(fx["w1_ulen"][k]) + int(fx["w1_vlen"][k])) * 2.0 ** -53 * fx["w1_abs"][k]
        assert abs(d[k] - ref) <= bar, (name, d[k], ref, bar)
    assert d[names.index("equal")] == 0.0
    assert fx["w1_ulen"][names.index("len256")] == 256
    # a pair alone: a float, the batch's bits
    k = names.index("lengths")
    alone = S.wasserstein_distance_norm(fx["w1_u"][k, :fx["w1_ulen"][k]],
                                        fx["w1_v"][k, :fx["w1_vlen"][k]])
    assert isinstance(alone, float) and same_bits(alone, d[k])


def test_stamp_metrics_is_the_chain_and_batch_invariant(fx, S):
    import torch
    o, r = fx["stamps"][np.repeat(np.arange(8), 5)], fx["stamps"][8:]
    co, cr = fx["stamp_center"][np.repeat(np.arange(8), 5)], fx["stamp_center"][8:]
    fo, fr = fx["stamp_fwhm"][np.repeat(np.arange(8), 5)], fx["stamp_fwhm"][8:]
    m = S.stamp_metrics(o, r, co, cr, fo, fr)
    # the five separate calls
    po, lo = S.radial_profile(o, co)
    pr, lr = S.radial_profile(r, cr)
    fito, _, _, iero, nfo = S.fit_radprof(po, fo, lengths=lo, full=True)
    fitr, _, _, ierr, nfr = S.fit_radprof(pr, fr, lengths=lr, full=True)
    wd = S.wasserstein_distance_norm(fito, fitr, lo, lr)
    for got, want in ((m["orig_radprof"], po), (m["restored_radprof"], pr),
                      (m["fitted_orig"], fito), (m["fitted_restored"], fitr)):
        w = want.shape[1]
        assert same_bits(got[:, :w], want) and np.all(np.isnan(got[:, w:]))
    np.testing.assert_array_equal(m["orig_len"], lo)
    np.testing.assert_array_equal(m["restored_len"], lr)
    np.testing.assert_array_equal(m["ier"], np.stack((iero, ierr), 1))
    np.testing.assert_array_equal(m["nfev"], np.stack((nfo, nfr), 1))
    assert same_bits(m["wd"], wd)
    # a batch is its images one by one
    for k in (0, 13, 39):
        one = S.stamp_metrics(o[k:k + 1], r[k:k + 1], co[k:k + 1], cr[k:k + 1], fo[k:k + 1],
                              fr[k:k + 1])
        for key in ("orig_radprof", "restored_radprof", "fitted_orig", "fitted_restored"):
            w = one[key].shape[1]
            assert same_bits(one[key][0], m[key][k, :w]), (key, k)
        for key in ("orig_len", "restored_len", "ier", "nfev"):
            np.testing.assert_array_equal(one[key][0], m[key][k])
        assert same_bits(one["wd"][0], m["wd"][k])
    dev = S.stamp_metrics(o[:2], r[:2], co[:2], cr[:2], fo[:2], fr[:2], device_out=True)
    assert all(torch.is_tensor(v) and v.is_cuda for v in dev.values())
    assert same_bits(dev["wd"].cpu().numpy(), m["wd"][:2])
