"""Host statement of the star-stamp metrics in numpy and scipy:
what the device kernels of bsgp_stamps.hip are compared with.

* ``radial_profile``: the mean of the pixels whose truncated distance from
  ``center`` is k, ``center[0]`` measured along the rows (axis 0).
* ``fit_gauss1d``: a three-parameter Gaussian fitted to (0 .. len-1, profile)
  by ``scipy.optimize.leastsq`` (MINPACK lmder) with an analytic Jacobian, the
  settings and the stddev bound of astropy 4.3.1's ``LevMarLSQFitter`` on a
  ``Gaussian1D``.  Modelled on astropy's source, pinned to scipy.
* ``wasserstein1``: ``scipy.stats.wasserstein_distance`` of two unweighted
  samples, written out.
"""
import numpy as np

TINY32 = float(np.finfo(np.float32).tiny)
FTOL, XTOL, GTOL, MAXFEV, FACTOR = 1.49012e-8, 1e-7, 0.0, 100, 100


def radial_profile(data, center):
    d = np.asarray(data).astype(np.float64)
    rows, cols = np.indices(d.shape)
    r = np.sqrt((rows - center[0]) ** 2 + (cols - center[1]) ** 2).astype(int)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.bincount(r.ravel(), d.ravel()) / np.bincount(r.ravel())


def sigma0(fwhm):
    return fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))


def model(p, x):
    a, m, s = p
    s = np.fmax(s, TINY32)
    with np.errstate(all="ignore"):
        return a * np.exp(-0.5 * (x - m) ** 2 / (s * s))


def fit_gauss1d(prof, fwhm):
    """Returns dict(fitted, params, perr, ier, nfev, nonfinite_trials); a profile
    shorter than 3 or with a non-finite value gives ier 0 and NaNs."""
    from scipy.optimize import leastsq
    y = np.asarray(prof, np.float64)
    n = len(y)
    nan3 = np.full(3, np.nan)
    if n < 3 or not np.all(np.isfinite(y)):
        return dict(fitted=np.full(n, np.nan), params=nan3, perr=nan3.copy(), ier=0, nfev=0,
                    nonfinite_trials=0)
    x = np.arange(n).astype(np.float64)

    nonfinite = [0]  # trial points whose residuals are not all finite (rejected by lmder)

    def resid(p):
        r = model(p, x) - y
        nonfinite[0] += not np.all(np.isfinite(r))
        return r

    def jac(p):
        a, m, s = p
        with np.errstate(all="ignore"):
            d = x - m
            e = np.exp(-0.5 * d ** 2 / (s * s))
            return [e, a * e * d / (s * s), a * e * d ** 2 / (s * s * s)]

    p0 = [0.8 * np.max(y), 0.0, sigma0(fwhm)]
    with np.errstate(all="ignore"):
        p, cov, info, _, ier = leastsq(resid, p0, Dfun=jac, col_deriv=True, full_output=True,
                                       ftol=FTOL, xtol=XTOL, gtol=GTOL, maxfev=MAXFEV,
                                       factor=FACTOR)
    p = np.array([p[0], p[1], max(p[2], TINY32)])
    if cov is None or n <= 3:
        perr = nan3
    else:
        perr = np.sqrt(np.abs(np.diag(cov * (np.sum(info["fvec"] ** 2) / (n - 3)))))
    return dict(fitted=model(p, x), params=p, perr=perr, ier=int(ier), nfev=int(info["nfev"]),
                nonfinite_trials=nonfinite[0])


def wasserstein1(u, v):
    """(distance, sum of the terms' magnitudes); NaN for a non-finite value."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    if not (np.all(np.isfinite(u)) and np.all(np.isfinite(v))):
        return np.nan, np.nan
    us, vs = np.sort(u), np.sort(v)
    t = np.sort(np.concatenate([u, v]), kind="mergesort")
    dt = np.diff(t)
    cu = np.searchsorted(us, t[:-1], "right") / u.size
    cv = np.searchsorted(vs, t[:-1], "right") / v.size
    terms = np.abs(cu - cv) * dt
    return float(np.sum(terms)), float(np.sum(np.abs(terms)))


# ---- comparisons the CPU and the GPU tests share
def fit_bar(fx, i):
    """The bars of fit i of the fixture (tests/test_gpu_stamp_metrics.py explains them)."""
    return (256.0 * float(fx["fit_resp"][i]) + 64 * 2.0 ** -53,
            256.0 * float(fx["fit_resp_perr"][i]) + 64 * 2.0 ** -53)


def same_bits(a, b):
    """Equal bit for bit, any NaN matching any NaN (numpy's 0 / 0 carries the
    sign bit, the device's does not)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b))
                and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))


def check_fit(fx, i, fitted, perr, ier, nfev):
    """ier / nfev equal, fitted and perr within their bars; returns the largest
    difference as a fraction of its bar."""
    n = int(fx["fit_len"][i])
    assert (int(ier), int(nfev)) == (int(fx["fit_ier"][i]), int(fx["fit_nfev"][i])), i
    bar_f, bar_p = fit_bar(fx, i)
    assert bar_f < 1e-9 and bar_p < 1e-9
    ref = fx["fit_fitted"][i, :n]
    df = np.max(np.abs(np.asarray(fitted)[:n] - ref)) / np.max(np.abs(ref))
    assert df <= bar_f, (i, df, bar_f)
    rp = fx["fit_perr"][i]
    if not np.all(np.isfinite(rp)):
        assert same_bits(np.isnan(perr), np.isnan(rp)), (i, perr, rp)
        return df / bar_f
    dp = np.max(np.abs(np.asarray(perr) - rp)) / np.max(np.abs(rp))
    assert dp <= bar_p, (i, dp, bar_p)
    return max(df / bar_f, dp / bar_p)
