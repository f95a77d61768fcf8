"""Writes tests/golden/stampmetrics_cases.npz: inputs and expected results of
the star-stamp metrics, computed by tests/stamps_ref.py (numpy
and scipy only).

    python tests/golden/make_golden_stampmetrics.py

Contents:
* ``stamps`` [48, 31, 31]: the 8 cutouts of ref_stamps31.npz minus their
  ``bkg`` (0..7), then the 40 restored stamps minus their median (8 + 5 i + k),
  with the centres (crude moment centroids, (row, column)) and FWHMs (second
  moments) used, their profiles, and the fit of every profile;
* synthetic profile cases (``pc_*``: float32 images, widened by the tests);
* synthetic fit cases appended to the 48 (``fit_*`` rows 48 ..), then four stamp
  profiles started from a FWHM of 0.06 to 0.08 pixels, three of which pass
  through trial points with non-finite residuals (``fit_nonfinite_trials``);
* for every fit the rounding response: the largest relative change of the
  fitted profile, and of perr, over 16 random perturbations of the profile by
  at most 4 ulp per value.  ier and nfev must not change and both responses
  must stay below 1e-10, or this script fails: replace the case then;
* Wasserstein cases: the fitted profiles of each (cutout, restored) pair, then
  synthetic ones, with the distance and the sum of the terms' magnitudes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import stamps_ref as R  # noqa: E402

RCAP = 256


def moments(d):
    """Crude centre (row, column) and FWHM from the positive part's moments."""
    w = np.clip(d, 0.0, None)
    rows, cols = np.indices(d.shape)
    s = w.sum()
    c0, c1 = (rows * w).sum() / s, (cols * w).sum() / s
    var = 0.5 * (((rows - c0) ** 2 * w).sum() / s + ((cols - c1) ** 2 * w).sum() / s)
    return (float(c0), float(c1)), float(2.0 * np.sqrt(2.0 * np.log(2.0)) * np.sqrt(var))


def pad(rows, fill=np.nan, width=RCAP):
    out = np.full((len(rows), width), fill)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def response(prof, fwhm, base, seed, rounds=16):
    """Largest relative change of (fitted, perr) over `rounds` perturbations
    from the stream of `seed` (more rounds repeat the first ones and go on)."""
    rng = np.random.default_rng(1000 + seed)
    fit_r, perr_r = 0.0, 0.0
    for _ in range(rounds):
        k = rng.integers(-4, 5, len(prof))
        f = R.fit_gauss1d(prof + k * np.spacing(prof), fwhm)
        if (f["ier"], f["nfev"]) != (base["ier"], base["nfev"]):
            return np.inf, np.inf  # the exit test is on an edge: not a usable case
        fit_r = max(fit_r, np.max(np.abs(f["fitted"] - base["fitted"])) / np.max(np.abs(base["fitted"])))
        if np.all(np.isfinite(base["perr"])):
            perr_r = max(perr_r, np.max(np.abs(f["perr"] - base["perr"])) / np.max(np.abs(base["perr"])))
    return fit_r, perr_r


def main():
    rng = np.random.default_rng(20240917)
    z = np.load(os.path.join(HERE, "ref_stamps31.npz"))
    cuts = [z[f"cut{i}"].astype(np.float64) - float(z[f"bkg{i}"]) for i in range(8)]
    rest = [z[f"x{i}_{k}"] - np.median(z[f"x{i}_{k}"]) for i in range(8) for k in range(5)]
    stamps = np.array(cuts + rest)
    out = {"stamps": stamps}
    # centre and FWHM of a stamp: its moments, or (where the fit from them ends
    # on the edge of an exit test, see response()) the moments rounded to 1/2,
    # 1/4 or 1/8 of a pixel (64 perturbations decide, the first 16 are recorded)
    ctr, fwhm = [], []
    for i, s in enumerate(stamps):
        c, f = moments(s)
        for q in (None, 2.0, 4.0, 8.0):
            cq = c if q is None else tuple(round(v * q) / q for v in c)
            p = R.radial_profile(s, cq)
            if max(response(p, f, R.fit_gauss1d(p, f), i, rounds=64)) < 1e-10:
                break
        else:
            raise SystemExit("no usable centre for a stamp")
        ctr.append(cq), fwhm.append(f)
    out["stamp_center"], out["stamp_fwhm"] = np.array(ctr), np.array(fwhm)
    profs = [R.radial_profile(s, c) for s, c in zip(stamps, ctr)]
    out["stamp_prof"], out["stamp_len"] = pad(profs), np.array([len(p) for p in profs], np.int32)

    # ---- synthetic profile cases: (shape, centre), float32 pixels of a wide range
    pcs = {
        "1x1": ((1, 1), (0.0, 0.0)), "1x7": ((1, 7), (0.0, 2.5)), "7x1": ((7, 1), (3.25, 0.0)),
        "5x9_offcentre": ((5, 9), (1.3, 6.6)), "corner": ((9, 11), (8.0, 10.0)),
        "outside": ((6, 5), (-3.5, 7.25)), "1x3_empty_bin0": ((1, 3), (1.5, 0.0)),
        "33x64": ((33, 64), (15.7, 30.2)), "128x128": ((128, 128), (63.5, 64.25)),
    }
    out["pc_names"] = np.array(sorted(pcs))
    for name, (shape, c) in pcs.items():
        img = (rng.standard_normal(shape) * np.exp(4.0 * rng.standard_normal(shape))).astype(np.float32)
        out[f"pc_img_{name}"], out[f"pc_center_{name}"] = img, np.array(c)
        out[f"pc_prof_{name}"] = R.radial_profile(img.astype(np.float64), c)
    assert np.isnan(out["pc_prof_1x3_empty_bin0"][0])

    # ---- fits: the 48 profiles, then synthetic ones
    fit_prof, fit_fwhm = list(profs), list(fwhm)
    x = np.arange(RCAP, dtype=np.float64)
    for n, a, m, s, noise, fw in [(3, 5.0, 0.2, 1.0, 0.0, 2.0), (4, 3.0, 0.0, 1.5, 0.01, 3.0),
                                  (12, 100.0, 0.5, 2.0, 0.5, 4.0), (40, 1.0, 0.0, 3.0, 0.02, 9.0),
                                  (65, 7.0, 1.0, 6.0, 0.05, 10.0), (130, 2.0, 0.0, 20.0, 0.01, 30.0),
                                  (256, 50.0, 3.0, 35.0, 0.3, 60.0), (22, -4.0, 0.0, 2.5, 0.05, 6.0)]:
        fit_prof.append(a * np.exp(-0.5 * (x[:n] - m) ** 2 / s ** 2) + noise * rng.standard_normal(n))
        fit_fwhm.append(fw)
    # stamp profiles started far too narrow (a FWHM of 0.07 pixels): the first
    # steps overshoot to trial points whose residuals are not finite, which lmder
    # must reject (actred stays -1) and answer by shrinking delta; at 0.06 the
    # Jacobian's last two columns vanish and lmder leaves with exit code 4
    narrow = [(0, 0.07), (8, 0.08), (45, 0.07), (3, 0.06)]
    for i, fw in narrow:
        fit_prof.append(profs[i]), fit_fwhm.append(fw)
    fits = [R.fit_gauss1d(p, f) for p, f in zip(fit_prof, fit_fwhm)]
    assert all(f["nonfinite_trials"] > 0 for f in fits[-4:-1]) and fits[-1]["ier"] == 4
    out["fit_nonfinite_trials"] = np.array([f["nonfinite_trials"] for f in fits], np.int32)
    resp = [response(p, f, b, i) for i, (p, f, b) in enumerate(zip(fit_prof, fit_fwhm, fits))]
    assert max(max(r) for r in resp) < 1e-10, resp
    assert sum(f["ier"] == 5 for f in fits) >= 3, [f["ier"] for f in fits]
    out["fit_prof"], out["fit_len"] = pad(fit_prof), np.array([len(p) for p in fit_prof], np.int32)
    out["fit_fwhm"] = np.array(fit_fwhm)
    out["fit_fitted"] = pad([f["fitted"] for f in fits])
    out["fit_params"] = np.array([f["params"] for f in fits])
    out["fit_perr"] = np.array([f["perr"] for f in fits])
    out["fit_ier"] = np.array([f["ier"] for f in fits], np.int32)
    out["fit_nfev"] = np.array([f["nfev"] for f in fits], np.int32)
    out["fit_resp"], out["fit_resp_perr"] = (np.array(v) for v in zip(*resp))
    # a singular R: a profile of zeros (amplitude 0: two Jacobian columns vanish)
    sing = R.fit_gauss1d(np.zeros(9), 3.0)
    assert np.all(np.isnan(sing["perr"]))
    out["sing_ier"], out["sing_nfev"] = np.int32(sing["ier"]), np.int32(sing["nfev"])
    out["sing_fitted"], out["sing_params"] = sing["fitted"], sing["params"]

    # ---- Wasserstein cases
    wu = [fits[i]["fitted"] for i in range(8) for _ in range(5)]
    wv = [fits[8 + j]["fitted"] for j in range(40)]
    a = rng.standard_normal(17)
    wu += [a, rng.standard_normal(9), np.array([1.0, 2.0, 2.0, 3.0, 2.0]), np.array([1.5]),
           -np.abs(rng.standard_normal(20)) - 1.0, rng.standard_normal(256) * 10.0,
           np.array([1.0, np.nan, 2.0]), np.array([3.0, 1.0])]
    wv += [a.copy(), rng.standard_normal(23), np.array([2.0, 2.0, 1.0, 4.0]), np.array([-0.25]),
           rng.standard_normal(33), rng.standard_normal(256) * 10.0 + 1.0,
           np.array([1.0, 2.0, 3.0]), np.array([np.inf, 2.0, 0.5])]
    d, dabs = zip(*(R.wasserstein1(u, v) for u, v in zip(wu, wv)))
    out["w1_names"] = np.array([f"pair{i}_{k}" for i in range(8) for k in range(5)]
                               + ["equal", "lengths", "ties", "single", "negative", "len256",
                                  "nan", "inf"])
    out["w1_u"], out["w1_ulen"] = pad(wu), np.array([len(u) for u in wu], np.int32)
    out["w1_v"], out["w1_vlen"] = pad(wv), np.array([len(v) for v in wv], np.int32)
    out["w1_d"], out["w1_abs"] = np.array(d), np.array(dabs)
    from scipy.stats import wasserstein_distance
    for u, v, di in zip(wu, wv, d):
        if np.isfinite(di):
            assert di == wasserstein_distance(u, v), (di, wasserstein_distance(u, v))
    assert d[40] == 0.0

    path = os.path.join(HERE, "stampmetrics_cases.npz")
    np.savez_compressed(path, **out)
    ier = out["fit_ier"]
    print(f"{path}: {os.path.getsize(path)} bytes; fits {len(ier)}, ier counts "
          f"{dict(zip(*np.unique(ier, return_counts=True)))}, nfev max {out['fit_nfev'].max()}, "
          f"response max {out['fit_resp'].max():.2e} (perr {out['fit_resp_perr'].max():.2e})")


if __name__ == "__main__":
    main()
