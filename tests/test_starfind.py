"""Star finding without a GPU: the numpy restatement
tests/starfind_ref.py on hand-made frames, the argument checks and the .coo
file of the product module, and the committed fixture against the restatement
that wrote it."""
import ast
import os

import numpy as np
import pytest

import localbkg_ref
import starfind_ref as ref
from conftest import GOLDEN, golden


def gauss(shape, x, y, amp, fwhm):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    s = fwhm * ref.FWHM_TO_SIGMA
    return amp * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))


def row_of(res, x, y):
    k = np.flatnonzero((res["ic"] == x) & (res["ir"] == y))
    assert len(k) == 1, (x, y, list(zip(res["ic"], res["ir"])))
    return int(k[0])


# ------------------------------------------------------------------ F1 to F3
def test_template_support_and_zero_mean():
    tp = ref.template(4.5)
    assert tp["R"] == 5 and tp["rap"] == pytest.approx(5.4)
    assert tp["n"] == int(np.sum(2 * tp["halfw"] + 1)) == len(tp["t"])
    assert np.all(tp["dx"] ** 2 + tp["dy"] ** 2 <= tp["rap"] ** 2)
    # row-major order
    key = tp["dy"] * 100 + tp["dx"]
    assert np.all(np.diff(key) > 0)
    assert abs(tp["t"].sum()) < 1e-13 and tp["tt"] == pytest.approx(np.sum(tp["t"] ** 2))
    one = ref.template(1.0, aprad=1.0)
    assert one["R"] == 1 and one["n"] == 5 and one["halfw"].tolist() == [0, 1, 0]
    import starfind
    mine = starfind.star_template(4.5)
    assert np.array_equal(mine["t"], tp["t"]) and mine["tt"] == tp["tt"]
    assert np.array_equal(mine["halfw"], tp["halfw"])


def test_single_gaussian_is_found_and_measured():
    """A noiseless Gaussian on a constant sky: one star, at its centre, with
    the flux and the moment FWHM of the Gaussian truncated at the aperture.
    The pixel sums differ from the integrals over the disc only by the disc's
    pixelated edge: a ring of about 2 pi rap half pixels at the edge's value
    exp(-u), u = rap^2 / (2 sigma^2) = 3.99, against the total 2 pi sigma^2:
    rap / 2 exp(-u) / sigma^2 = 1.4 % of the flux, and u times that in the
    second moment, half of it in its root: 2.7 %."""
    shape, fwhm, amp = (64, 64), 4.5, 1000.0
    img = 10.0 + gauss(shape, 32, 30, amp, fwhm)
    res = ref.find_stars(img, fwhm, noise=1.0)
    assert len(res["ic"]) == 1 and (res["ic"][0], res["ir"][0]) == (32, 30)
    assert res["status"][0] == 0 and res["nsat"][0] == 0
    assert res["bkg"][0] == pytest.approx(10.0, abs=1e-9)
    assert res["x"][0] == pytest.approx(32.0, abs=1e-9) and res["y"][0] == pytest.approx(30.0, abs=1e-9)
    assert res["corr"][0] == pytest.approx(1.0, abs=1e-12)
    assert res["amp"][0] == pytest.approx(amp, rel=1e-12)
    assert res["peak"][0] == pytest.approx(amp, rel=1e-9)
    tp = res["template"]
    g = np.exp(-(tp["dx"] ** 2 + tp["dy"] ** 2) / (2 * (fwhm * ref.FWHM_TO_SIGMA) ** 2))
    assert res["flux"][0] == pytest.approx(amp * g.sum(), rel=1e-12)
    sigma = fwhm * ref.FWHM_TO_SIGMA
    u = tp["rap"] ** 2 / (2 * sigma ** 2)
    assert res["flux"][0] == pytest.approx(2 * np.pi * sigma ** 2 * amp * (1 - np.exp(-u)), rel=0.014)
    want = fwhm * np.sqrt(1 - u * np.exp(-u) / (1 - np.exp(-u)))
    assert res["fwhm"][0] == pytest.approx(want, rel=0.027)
    print(f"flux / total {res['flux'][0] / (2 * np.pi * sigma ** 2 * amp):.4f} "
          f"(disc {1 - np.exp(-u):.4f}); fwhm {res['fwhm'][0]:.4f} (truncated {want:.4f})")


def test_maps_validity():
    """F2: a pixel whose support leaves the frame, holds a non-finite pixel or
    a masked one is NaN in both maps; a saturated pixel invalidates nothing."""
    rng = np.random.default_rng(0)
    img = 100 + rng.standard_normal((20, 24))
    img[10, 12] = np.inf
    mask = np.zeros(img.shape, np.uint8)
    mask[4, 5] = 1
    tp = ref.template(2.0)  # rap 2.4, R 2
    corr, amp, _ = ref.maps(img, tp, mask)
    want = np.zeros(img.shape, bool)
    want[2:-2, 2:-2] = True
    for (y, x) in ((10, 12), (4, 5)):
        for dy, dx in zip(tp["dy"], tp["dx"]):
            want[y - dy, x - dx] = False
    assert np.array_equal(~np.isnan(amp), want) and np.array_equal(~np.isnan(corr), want)
    flat = ref.maps(np.full((9, 9), 7.0), tp)
    assert flat[0][4, 4] == 0.0 and flat[1][4, 4] == 0.0  # var = 0: corr 0
    for small in ((1, 1), (4, 9), (9, 4)):
        assert np.isnan(ref.maps(np.ones(small), tp)[1]).all()


def test_tie_rule_on_a_flat_top():
    """F4: among equal amplitudes the first pixel in raster order is the
    candidate (strictly above earlier pixels, >= later ones)."""
    amp = np.zeros((7, 7))
    amp[2, 2:4] = 5.0
    amp[3, 2:4] = 5.0   # a 2 x 2 plateau
    amp[5, 5] = 5.0
    amp[0, 0] = np.nan  # not valid: ignored by its neighbours
    amp[0, 1] = 1.0
    corr = np.ones((7, 7))
    st = np.full((7, 7), 10.0)
    ir, ic, _ = ref.candidates(corr, amp, st, 1.0, 1.0, c_min=0.4, thresh=2.0, peak_hw=1)
    assert list(zip(ir.tolist(), ic.tolist())) == [(0, 1), (2, 2), (5, 5)]
    # a saturated core: one star on the plateau, its brightest pixel the first
    # of the 3 x 3 plateau in raster order, sqrt(2) > dxy from the centroid
    img = np.minimum(20.0 + gauss((48, 48), 24, 24, 5000.0, 4.0), 3000.0)
    assert np.count_nonzero(img == 3000.0) == 9
    res = ref.find_stars(img, 4.0, noise=1.0, sat_level=3000.0, anrad1=10, anrad2=14)
    assert len(res["ic"]) == 1
    assert res["nsat"][0] == 9 and res["status"][0] == ref.OFF_CENTRE
    assert res["x"][0] == pytest.approx(24.0, abs=1e-9) and res["d2"][0] == pytest.approx(2.0)
    assert res["peak"][0] == pytest.approx(3000.0 - res["bkg"][0])


def test_rejection_bits():
    """F8: BAD_FLUX under a sky above the star, FEW_SKY (and with its NaN sky
    BAD_FLUX) when the annulus is masked away, SKY_OVER_CAP over 8192 values."""
    shape = (64, 64)
    yy, xx = np.mgrid[:64, :64]
    d2 = (xx - 32) ** 2 + (yy - 32) ** 2
    ann = (d2 >= 100) & (d2 <= 196)
    star = 10.0 + gauss(shape, 32, 32, 300.0, 3.0)
    kw = dict(fwhm=3.0, noise=1.0, anrad1=10, anrad2=14)
    res = ref.find_stars(star, **kw)
    assert res["status"][row_of(res, 32, 32)] == 0
    res = ref.find_stars(np.where(ann, 1000.0, star), **kw)
    k = row_of(res, 32, 32)
    assert res["status"][k] & ref.BAD_FLUX and res["flux"][k] < 0 and res["bkg"][k] == 1000.0
    mask = ann.astype(np.uint8)
    ys, xs = np.nonzero(ann)
    mask[ys[:9], xs[:9]] = 0
    res = ref.find_stars(star, mask=mask, **kw)
    k = row_of(res, 32, 32)
    assert res["status"][k] == ref.FEW_SKY | ref.BAD_FLUX and np.isnan(res["bkg"][k])
    mask[ys[9], xs[9]] = 0  # the tenth value: a sky
    res = ref.find_stars(star, mask=mask, **kw)
    assert res["status"][row_of(res, 32, 32)] == 0
    big = 10.0 + gauss((140, 140), 70, 70, 300.0, 3.0)
    res = ref.find_stars(big, 3.0, noise=1.0, anrad1=20, anrad2=60)
    k = row_of(res, 70, 70)
    assert res["nsky"][k] > ref.MAX_SKY
    assert res["status"][k] == ref.SKY_OVER_CAP | ref.BAD_FLUX and np.isnan(res["flux"][k])


def test_max_stars_keeps_the_first_in_raster_order():
    fx = golden("starfind_cases.npz")
    kw = ast.literal_eval(str(fx["lattice_kw"]))
    full = ref.find_stars(fx["lattice_img"], **kw)
    cut = ref.find_stars(fx["lattice_img"], max_stars=8, **kw)
    assert full["frame_status"] == 0 and cut["frame_status"] == ref.OVER_CAP
    assert np.array_equal(cut["ic"], full["ic"][:8]) and np.array_equal(cut["flux"], full["flux"][:8])
    order = full["ir"].astype(np.int64) * 96 + full["ic"]
    assert np.all(np.diff(order) > 0) and len(order) == int(fx["lattice_n"])


# ---------------------------------------------------------------------- F9
def _sel(x, y, flux, **kw):
    n = len(x)
    a = dict(peak=np.asarray(flux, float), nsat=np.zeros(n, int), status=np.zeros(n, int),
             shape=(200, 200), hw=15, iso_radius=10.0, min_flux=100.0, rat_thresh=0.25)
    a.update(kw)
    return ref.select_psf_stars(np.asarray(x, float), np.asarray(y, float), np.asarray(flux, float), **a)


def test_selection_boundaries():
    # exactly iso_radius away (6, 8, 10): a rival; a hair beyond: none
    sel, el, rank = _sel([50, 56], [50, 58], [1000, 1000])
    assert not el.any() and len(sel) == 0 and rank.tolist() == [-1, -1]
    sel, el, _ = _sel([50, 56], [50, np.nextafter(58, 59)], [1000, 1000])
    assert el.all()
    # exactly rat_thresh of the flux: a rival of the bright one; below: not
    _, el, _ = _sel([50, 56], [50, 58], [1000, 250])
    assert el.tolist() == [False, False]
    _, el, _ = _sel([50, 56], [50, 58], [1000, np.nextafter(250, 0)])
    assert el.tolist() == [True, False]  # the bright one is still the faint one's rival
    # equal fluxes: the smaller index ranks first; the cut at npsf_max
    x = [30, 60, 90, 120, 150]
    sel, el, rank = _sel(x, [100] * 5, [500, 900, 500, 900, 700], npsf_max=3)
    assert el.all() and rank.tolist() == [3, 0, 4, 1, 2] and sel.tolist() == [1, 3, 4]
    # the other conditions
    _, el, _ = _sel(x, [100] * 5, [99, 100, 500, 500, 500], nsat=np.array([0, 0, 1, 0, 0]),
                    status=np.array([0, 0, 0, ref.OFF_CENTRE, 0]), peak=np.array([1, 1, 1, 1, 9e4]),
                    max_peak=5e4)
    assert el.tolist() == [False, True, False, False, False]
    # the box rule: floor(x + 0.5) - hw >= 0 and + hw < W
    _, el, _ = _sel([14.4, 14.5, 184.4, 184.5], [40, 80, 120, 160], [500] * 4)
    assert el.tolist() == [False, True, True, False]
    # a rejected star is nobody's rival
    _, el, _ = _sel([50, 56], [50, 58], [1000, 1000], status=np.array([0, ref.BAD_FLUX]))
    assert el.tolist() == [True, False]
    sel, el, rank = _sel([], [], [])
    assert len(sel) == 0 and len(el) == 0


# ------------------------------------------------------------- the product's
def test_argument_checks():
    import starfind as sf
    c = sf.check_find_args((40, 56), 2.5)
    assert (c["batched"], c["B"], c["R"], c["noise_mode"], c["max_stars"]) == (False, 1, 3, "number", 16384)
    count = sum(400 <= dx * dx + dy * dy <= 625 for dx in range(-25, 26) for dy in range(-25, 26))
    assert c["annulus_pixels"] == sf.annulus_pixels(20.0, 25.0) == count and not c["sky_over_cap"]
    assert not c["empty"]
    assert sf.check_find_args((3, 40, 56), 2.5, (3,))["noise_mode"] == "frame"
    assert sf.check_find_args((3, 40, 56), 2.5, (40, 56))["noise_mode"] == "map"
    assert sf.check_find_args((3, 40, 56), 2.5, (3, 40, 56))["noise_mode"] == "map"
    assert sf.check_find_args((6, 56), 2.5)["empty"] and sf.check_find_args((1, 1), 2.5)["empty"]
    assert sf.check_find_args((200, 200), 3.0, anrad1=20, anrad2=60)["sky_over_cap"]
    assert sf.check_find_args((9, 9), 13.3)["R"] == 15
    for bad, match in ((dict(image_shape=(5,)), "image must be"),
                       (dict(fwhm=0.0), "fwhm"), (dict(fwhm=13.4), "MAX_R"),
                       (dict(aprad=-1.0), "aprad"), (dict(anrad1=25, anrad2=25), "anrad1 < anrad2"),
                       (dict(anrad2=2000.0), "anrad2"), (dict(peak_hw=4), "peak_hw"),
                       (dict(peak_hw=1.0), "peak_hw"), (dict(max_stars=0), "max_stars"),
                       (dict(max_stars=16385), "max_stars"), (dict(bkg_alg="mod"), "bkg_alg"),
                       (dict(noise_shape=(4,)), "noise shape"), (dict(mask_shape=(40, 55)), "mask"),
                       (dict(sat_level="x"), "sat_level"), (dict(dxy=-1.0), "dxy"),
                       (dict(c_min=float("nan")), "c_min")):
        kw = dict(image_shape=(40, 56), fwhm=2.5)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            sf.check_find_args(**kw)
    s = sf.check_select_args(fwhm=4.0)
    assert s["iso_radius"] == 12.0 and s["hw"] == 15 and s["npsf_max"] == 100
    for bad, match in ((dict(hw=-1), "hw"), (dict(npsf_max=1.5), "npsf_max"), (dict(), "iso_radius"),
                       (dict(iso_radius=-2.0), "iso_radius"), (dict(max_peak="x", fwhm=4.0), "max_peak")):
        with pytest.raises(ValueError, match=match):
            sf.check_select_args(**bad)
    assert (sf.REJECTED, sf.OVER_CAP) == (ref.REJECTED, ref.OVER_CAP)
    assert (sf.MAX_R, sf.MAX_STARS, sf.MAX_SKY, sf.MIN_SKY) == (ref.MAX_R, ref.MAX_STARS, ref.MAX_SKY,
                                                             ref.MIN_SKY)
    assert (sf.SKY_SIGMA, sf.SKY_MAXITERS) == (ref.SKY_SIGMA, ref.SKY_MAXITERS)


def test_coo_round_trip(tmp_path):
    import starfind as sf
    t = np.array([[10.25, 20.5, 1234.5678901234567, 99.1, 0], [1 / 3, 2 / 3, 1e-3, -4.0, 7],
                  [5.0, 6.0, np.nan, np.nan, 0]])
    p = str(tmp_path / "frame.coo")
    sf.write_coo(p, t)
    back = sf.read_coo(p)
    assert np.array_equal(back, t, equal_nan=True)
    lines = open(p).read().splitlines()
    assert len(lines) == 3 + len(t) and lines[2] == sf.COO_HEADER
    assert all(len(l.split()) == 5 for l in lines[3:])
    # the application's reader
    assert np.array_equal(np.loadtxt(p, skiprows=3), t, equal_nan=True)
    sf.write_coo(p, t, index_base=1)
    assert np.loadtxt(p, skiprows=3)[0, :2].tolist() == [11.25, 21.5]
    assert np.allclose(sf.read_coo(p, index_base=1)[:2], t[:2], rtol=0, atol=1e-15)
    sf.write_coo(p, np.zeros((0, 5)))
    assert sf.read_coo(p).shape == (0, 5)
    with pytest.raises(ValueError, match=r"\[m, 5\]"):
        sf.write_coo(p, np.zeros((3, 4)))


# --------------------------------------------------------------------- sky
def test_clipping_is_the_local_backgrounds():
    rng = np.random.default_rng(3)
    for n, tail in ((10, 0), (251, 5), (708, 40), (2000, 300)):
        v = 100 + 3 * rng.standard_normal(n)
        v[:tail] += rng.uniform(20, 400, tail)
        s = np.sort(v)
        assert ref.clip_sorted(s) == localbkg_ref.clip_sorted(s, 3.0, 10)
    # the three estimators on one annulus
    img = 100 + 3 * rng.standard_normal((64, 64))
    s = ref.annulus_values(img, 30, 31, 8.0, 12.0)
    lo, hi, _, med, mean, sd, _ = ref.clip_sorted(s)
    assert ref.sky(img, 30, 31, 8.0, 12.0, "median")["bkg"] == med
    assert ref.sky(img, 30, 31, 8.0, 12.0, "mean")["bkg"] == mean
    assert ref.sky(img, 30, 31, 8.0, 12.0, "mode")["bkg"] == localbkg_ref.mode_estimate(mean, med, sd)
    # the annulus: inclusive at both radii, inside the frame only
    assert len(s) == np.count_nonzero([(64 <= dx * dx + dy * dy <= 144)
                                       for dx in range(-12, 13) for dy in range(-12, 13)])
    assert len(ref.annulus_values(img, 0, 0, 8.0, 12.0)) < len(s) / 3


def test_fixture_is_the_restatements():
    """tests/golden/starfind_cases.npz holds what the restatement makes of its
    scene today."""
    fx = golden("starfind_cases.npz")
    kw = ast.literal_eval(str(fx["scene_kw"]))
    res = ref.find_stars(fx["scene_img"], mask=fx["scene_mask"], **kw)
    for c in ref.FCOLS + ("ic", "ir", "nsat", "status"):
        assert np.array_equal(res[c], fx["scene_" + c], equal_nan=True), c
    assert os.path.getsize(os.path.join(GOLDEN, "starfind_cases.npz")) < 1 << 20
    seen = int(res["status"].max() | res["status"].min())
    assert np.any(res["status"] == 0) and np.any(res["status"] & ref.OFF_CENTRE), seen


def test_c_abi_refuses_bad_arguments_on_the_host():
    """The four entry points validate before they touch a device."""
    import _bsgp
    L = _bsgp.lib()
    hw = np.zeros(33, np.int32)
    rc = L.bsgp_star_maps(None, 1, 1, 8, 8, None, None, hw.ctypes.data, 16, 1.0, None, None, None)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and b"15" in L.bsgp_last_error()
    hw[1] = 3
    rc = L.bsgp_star_maps(None, 1, 1, 8, 8, None, None, hw.ctypes.data, 2, 1.0, None, None, None)
    assert rc == _bsgp.BSGP_ERR_ARG and b"halfw" in L.bsgp_last_error()
    hw[1] = 1
    rc = L.bsgp_star_maps(None, 1, 1, 8, 8, None, None, hw.ctypes.data, 1, 1.0, None, None, None)
    assert rc == _bsgp.BSGP_ERR_ARG and b"tmpl" in L.bsgp_last_error()
    t = np.ones(5)
    rc = L.bsgp_star_maps(None, 1, 1, 8, 8, None, t.ctypes.data, hw.ctypes.data, 1, 0.0, None, None,
                          None)
    assert rc == _bsgp.BSGP_ERR_ARG and b"tt" in L.bsgp_last_error()
    rc = L.bsgp_star_peaks(None, 1, 1, 8, 8, None, None, t.ctypes.data, hw.ctypes.data, 1, 1.0, None,
                           0, 0.4, 2.0, 4, 8, None, None, None, None)
    assert rc == _bsgp.BSGP_ERR_ARG and b"peak_hw" in L.bsgp_last_error()
    rc = L.bsgp_star_peaks(None, 1, 1, 8, 8, None, None, t.ctypes.data, hw.ctypes.data, 1, 1.0, None,
                           0, 0.4, 2.0, 1, 16385, None, None, None, None)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED
    rc = L.bsgp_star_measure(None, 1, 1, 8, 8, None, None, None, hw.ctypes.data, 1, None, None, 4,
                             25.0, 20.0, 0, 3.0, 10, 10, 0, 0.0, 1.0, None, None, None)
    assert rc == _bsgp.BSGP_ERR_ARG and b"anrad1 < anrad2" in L.bsgp_last_error()
    rc = L.bsgp_star_measure(None, 1, 1, 8, 8, None, None, None, hw.ctypes.data, 1, None, None, 4,
                             20.0, 25.0, 3, 3.0, 10, 10, 0, 0.0, 1.0, None, None, None)
    assert rc == _bsgp.BSGP_ERR_ARG and b"bkg_alg" in L.bsgp_last_error()
    rc = L.bsgp_star_select(None, None, None, 1, 4, 8, 8, -1, 100.0, 0, 0.0, 0.2, 12.0, 100, None,
                            None, None, None)
    assert rc == _bsgp.BSGP_ERR_ARG and b"hw" in L.bsgp_last_error()
    rc = L.bsgp_star_select(None, None, None, 0, 4, 8, 8, 15, 100.0, 0, 0.0, 0.2, 12.0, 100, None,
                            None, None, None)
    assert rc == 0  # B == 0: a no-op that follows no pointer


def test_seeing_is_the_median_inside_the_limits():
    import starfind as sf
    cols = dict(status=np.array([0, 0, 0, ref.BAD_FLUX, 0, 0]),
                fwhm=np.array([3.0, 4.0, 5.0, 4.0, 12.0, 4.5]),
                peak=np.array([1000.0, 1000.0, 1000.0, 1000.0, 1000.0, 100.0]),
                x=np.array([50.0, 50.0, 50.0, 50.0, 50.0, 50.0]),
                y=np.array([50.0, 50.0, 2.0, 50.0, 50.0, 50.0]))
    assert ref.seeing(cols, (100, 100)) == 3.5
    assert np.isnan(ref.seeing(cols, (100, 100), min_peak=1e6))
    assert sf.StarList.seeing.__defaults__ == ref.seeing.__defaults__
