"""GPU tests of starfind.find_stars and starfind.select_psf_stars
(bsgp_star_maps / _peaks / _measure / _select) against the numpy
restatement tests/starfind_ref.py.

What is compared.  The maps are equal bit for bit at every pixel: device and
restatement add the same terms in the support's order.  The candidate list,
its order, ic, ir, nsat and status are equal exactly (the fixture's generator
asserts that no decision sits on its bound).  The sky differs by the summation
order of its mean and standard deviation and is held to the bar of the local
background (starfind_ref.sky: 0 for the median, which is exact).  Every other
float column is equal bit for bit to the restatement's F7 evaluated with the
device's sky.  Selection is exact."""
import ast
import os
import warnings

import numpy as np
import pytest

import starfind_ref as ref
from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sf():
    import _bsgp
    _bsgp.require_gpu()
    import starfind
    return starfind


@pytest.fixture(scope="module")
def fx():
    return golden("starfind_cases.npz")


def kwargs(fx, name):
    return ast.literal_eval(str(fx[name]))


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def compare(stars, img, mask=None, **kw):
    """The device's StarList of one frame against the restatement."""
    want = ref.find_stars(img, mask=mask, **kw)
    assert stars.n == len(want["ic"]), (stars.n, len(want["ic"]))
    for c in ("ic", "ir", "nsat", "status"):
        assert same(stars[c], want[c]), (c, stars[c], want[c])
    assert stars.frame_status == want["frame_status"]
    assert same(np.isnan(stars.bkg), np.isnan(want["bkg"]))
    fin = np.isfinite(want["bkg"])
    err = np.abs(stars.bkg[fin] - want["bkg"][fin])
    if fin.any():
        print(f"sky: largest |device - restatement| {err.max():.3e}, bar there "
              f"{want['bar'][fin][np.argmax(err)]:.3e}")
    assert np.all(err <= want["bar"][fin]), (err, want["bar"][fin])
    given = ref.find_stars(img, mask=mask, bkg=stars.bkg, **kw)
    for c in ("x", "y", "flux", "peak", "fwhm", "corr", "amp"):
        assert same(stars[c], given[c]), (c, stars[c], given[c])
    assert same(stars.kept, (want["status"] & ref.REJECTED) == 0)
    assert same(stars.xcentroid, stars.x) and same(stars.ycentroid, stars.y)
    return want


# -------------------------------------------------------------------- maps
_MAPS = {}


def ref_maps(fx, fwhm, aprad):
    if (fwhm, aprad) not in _MAPS:
        tp = ref.template(fwhm, aprad)
        _MAPS[(fwhm, aprad)] = (tp, ) + ref.maps(fx["noise_frame"], tp)[:2]
    return _MAPS[(fwhm, aprad)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("R, fwhm, aprad", [(1, 1.0, 1.0), (4, 3.5, 1.2), (15, 13.0, 1.2)])
def test_maps_bit_equal(sf, fx, R, fwhm, aprad, dtype):
    """Every pixel of a 70 x 150 noise frame: every tile seam (tiles of 32 x 16)
    and the valid region's border."""
    tp, corr, amp = ref_maps(fx, fwhm, aprad)
    assert tp["R"] == R and (R != 1 or tp["rap"] == 1.0)
    img = fx["noise_frame"].astype(dtype)
    stars = sf.find_stars(img, fwhm, noise=30.0, aprad=aprad, return_maps=True)
    assert same(stars.corr_map, corr) and same(stars.amp_map, amp)
    assert np.count_nonzero(~np.isnan(amp)) == (70 - 2 * R) * (150 - 2 * R)


def test_maps_tiny_frames(sf):
    rng = np.random.default_rng(4)
    tp = ref.template(1.0, 1.0)
    img = rng.standard_normal((3, 3))
    stars = sf.find_stars(img, 1.0, noise=1.0, aprad=1.0, return_maps=True)
    corr, amp, _ = ref.maps(img, tp)
    assert same(stars.corr_map, corr) and same(stars.amp_map, amp)
    assert np.count_nonzero(~np.isnan(stars.amp_map)) == 1
    for shape, fwhm in (((1, 1), 1.0), ((4, 9), 2.0), ((9, 4), 2.0), ((30, 40), 13.0)):
        stars = sf.find_stars(rng.standard_normal(shape), fwhm, noise=1.0, return_maps=True)
        assert stars.n == 0 and len(stars) == 0 and stars.x.shape == (0,)
        assert np.isnan(stars.amp_map).all() and np.isnan(stars.corr_map).all()
        assert stars.table().shape == (0, 5) and np.isnan(stars.seeing())


# ------------------------------------------------------------------- scene
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_scene(sf, fx, dtype):
    kw = kwargs(fx, "scene_kw")
    img, mask = fx["scene_img"].astype(dtype), fx["scene_mask"]
    stars = sf.find_stars(img, mask=mask, **kw)
    want = compare(stars, img, mask, **kw)
    for c in ("ic", "ir", "nsat", "status"):
        assert same(stars[c], fx["scene_" + c])
    peaks = set(zip(stars.ic.tolist(), stars.ir.tolist()))
    assert {(28, 20), (10, 28), (13, 28), (3, 12)} <= peaks and (20, 33) not in peaks
    assert not any(y < 3 for _, y in peaks)
    assert np.any(want["nsat"] > 1) and np.any(want["status"] & ref.OFF_CENTRE)
    t = stars.table()
    assert t.shape == (int(stars.kept.sum()), 5) and same(t[:, 0], stars.x[stars.kept])
    assert stars.table(kept_only=False).shape == (stars.n, 5)


# --------------------------------------------------------------------- sky
@pytest.mark.parametrize("alg", ["mode", "median", "mean"])
@pytest.mark.parametrize("name", ["const", "sym", "skew"])
def test_sky_estimators(sf, fx, name, alg):
    """std 0, |mean - median| / std below and above 0.3; an annulus cut by the
    frame's corner (the star at (6, 6))."""
    kw = kwargs(fx, "sky_kw")
    img = fx["sky_" + name]
    stars = sf.find_stars(img, bkg_alg=alg, **kw)
    want = compare(stars, img, bkg_alg=alg, **kw)
    k = int(np.flatnonzero((want["ic"] == 6) & (want["ir"] == 6))[0])
    assert 10 <= want["nsky"][k] < sf.annulus_pixels(kw["anrad1"], kw["anrad2"]) / 2
    if alg == "median":
        assert same(stars.bkg, want["bkg"])


def test_sky_few_values_and_over_cap(sf, fx):
    kw = kwargs(fx, "sky_kw")
    img, mask = fx["sky_sym"], fx["sky_few_mask"]
    stars = sf.find_stars(img, mask=mask, **kw)
    want = compare(stars, img, mask, **kw)
    k = int(np.flatnonzero((stars.ic == 32) & (stars.ir == 32))[0])
    assert want["nsky"][k] == 6 and stars.status[k] & sf.FEW_SKY and np.isnan(stars.bkg[k])
    assert not stars.kept[k]
    yy, xx = np.mgrid[:140, :140]
    big = (10.0 + 300.0 * np.exp(-((xx - 70) ** 2 + (yy - 70) ** 2) / 3.0)).astype(np.float32)
    kw = dict(fwhm=3.0, noise=1.0, anrad1=20.0, anrad2=60.0)
    with pytest.warns(sf.StarCapWarning, match="SKY_OVER_CAP"):
        stars = sf.find_stars(big, **kw)
    compare(stars, big, **kw)
    k = int(np.flatnonzero((stars.ic == 70) & (stars.ir == 70))[0])
    assert stars.status[k] == sf.SKY_OVER_CAP | sf.BAD_FLUX and np.isnan(stars.bkg[k])


# --------------------------------------------------------------- numbering
def test_lattice_numbering_and_cap(sf, fx):
    kw = kwargs(fx, "lattice_kw")
    img = fx["lattice_img"]
    stars = sf.find_stars(img, **kw)
    compare(stars, img, **kw)
    order = stars.ir.astype(np.int64) * 96 + stars.ic
    assert stars.n == int(fx["lattice_n"]) and np.all(np.diff(order) > 0)
    assert len(set(order // 2048)) >= 4  # several chunks of the compaction
    with pytest.warns(sf.StarCapWarning, match="max_stars"):
        cut = sf.find_stars(img, max_stars=8, **kw)
    assert cut.n == 8 and cut.frame_status == sf.OVER_CAP and stars.frame_status == 0
    for c in sf.FCOLS + sf.ICOLS:
        assert same(cut[c], stars[c][:8]), c


# ------------------------------------------------------------------- batch
def test_batch_gives_each_frame_its_own_bits(sf, fx):
    kw = kwargs(fx, "batch_kw")
    img, noise, nmap = fx["batch_img"], fx["batch_noise"], fx["batch_nmap"].astype(np.float64)
    for nz in (noise, nmap):
        both = [sf.find_stars(img, noise=nz, **kw) for _ in range(2)]
        assert len(both[0]) == 3 and both[0][1].n == 0  # the constant frame: var = 0
        for b in range(3):
            alone = sf.find_stars(img[b], noise=nz[b], **kw)
            assert alone.n == both[0][b].n and (b == 1 or alone.n > 0)
            for c in sf.FCOLS + sf.ICOLS:
                assert same(alone[c], both[0][b][c]) and same(both[0][b][c], both[1][b][c]), (b, c)
            compare(both[0][b], img[b], noise=nz[b], **kw)
    shared = sf.find_stars(img, noise=nmap[0], **kw)  # one map for every frame
    assert same(shared[2].flux, sf.find_stars(img[2], noise=nmap[0], **kw).flux)
    dev = sf.find_stars(img, noise=nmap, device_out=True, **kw)
    assert dev[0].x.is_cuda and same(dev[0]["x"], both[0][0].x) and dev.fcols.shape[0] == 3
    assert same(dev[2].kept.cpu().numpy(), both[0][2].kept)


# --------------------------------------------------------------- selection
def check_select(sf, x, y, flux, shape=(200, 200), fwhm=4.0, peak=None, nsat=None, status=None, **kw):
    n = len(x)
    peak = np.asarray(flux, float) if peak is None else peak
    nsat = np.zeros(n, np.int32) if nsat is None else nsat
    status = np.zeros(n, np.int32) if status is None else status
    stars = sf.StarList.from_columns(x, y, flux, shape, fwhm=fwhm, peak=peak, nsat=nsat, status=status)
    sel, el, rank = sf.select_psf_stars(stars, **kw)
    wsel, wel, wrank = ref.select_psf_stars(stars.x, stars.y, stars.flux, stars.peak, stars.nsat,
                                            stars.status, shape, fwhm=fwhm, **kw)
    assert same(sel, wsel) and same(el, wel) and same(rank, wrank), (sel, wsel)
    return sel, el, rank


def test_selection_equals_the_restatement(sf):
    sel, el, rank = check_select(sf, [], [], [])
    assert sel.shape == (0,) and el.shape == (0,)
    sel, el, _ = check_select(sf, [100.0], [100.0], [500.0])
    assert sel.tolist() == [0]
    rng = np.random.default_rng(9)
    n = 300  # two staged tiles, two workgroups
    x, y = rng.uniform(0, 400, n), rng.uniform(0, 400, n)
    flux = rng.uniform(50, 5000, n)
    flux[10:20] = flux[20:30]  # equal fluxes: ranked by index
    status = np.where(rng.random(n) < 0.2, rng.integers(1, 16, n), 0).astype(np.int32)
    nsat = (rng.random(n) < 0.1).astype(np.int32)
    for kw in (dict(), dict(npsf_max=20, max_peak=3000.0), dict(iso_radius=40.0, rat_thresh=0.5, hw=8)):
        sel, el, rank = check_select(sf, x, y, flux, (400, 400), peak=flux * 0.9, nsat=nsat,
                                     status=status, **kw)
        assert 0 < len(sel) <= kw.get("npsf_max", 100)
    assert el.any() and not el.all()


def test_selection_boundaries(sf):
    kw = dict(iso_radius=10.0, rat_thresh=0.25)
    _, el, _ = check_select(sf, [50, 56], [50, 58], [1000, 1000], **kw)  # exactly iso_radius
    assert not el.any()
    _, el, _ = check_select(sf, [50, 56], [50, np.nextafter(58, 59)], [1000, 1000], **kw)
    assert el.all()
    _, el, _ = check_select(sf, [50, 56], [50, 58], [1000, 250], **kw)  # exactly rat_thresh
    assert el.tolist() == [False, False]
    _, el, _ = check_select(sf, [50, 56], [50, 58], [1000, np.nextafter(250, 0)], **kw)
    assert el.tolist() == [True, False]
    sel, el, rank = check_select(sf, [30, 60, 90, 120, 150], [100] * 5, [500, 900, 500, 900, 700],
                                 npsf_max=3, **kw)
    assert rank.tolist() == [3, 0, 4, 1, 2] and sel.tolist() == [1, 3, 4]
    # a star whose box leaves the frame
    _, el, _ = check_select(sf, [14.4, 14.5, 184.4, 184.5], [40, 80, 120, 160], [500] * 4, **kw)
    assert el.tolist() == [False, True, True, False]
    _, el, _ = check_select(sf, [100, 100], [14.4, 185.0], [500, 500], **kw)
    assert el.tolist() == [False, False]


# -------------------------------------------------------------- end to end
def test_frame_to_psf_and_stamps(sf):
    """tests/golden/SUBDIV_ORIGIMG.fits: find_stars equals the restatement, the
    chosen stars carry a non-singular fit_psf, sgp_star_stamps takes the table's
    positions."""
    import fits_io
    import psf_calculate as pc
    import stamps
    _, img = fits_io.read_fits(os.path.join(GOLDEN, "SUBDIV_ORIGIMG.fits"))
    _, psf = fits_io.read_fits(os.path.join(GOLDEN, "psfccfbrd210048_1_1_img.fits"))
    img = np.ascontiguousarray(np.asarray(img).astype(np.float32))
    kw = dict(fwhm=4.5, noise=9.8, thresh=3.0)
    stars = sf.find_stars(img, **kw)
    compare(stars, img, **kw)
    assert stars.n >= 30 and stars.kept.sum() >= 20
    assert 2.6 < stars.seeing(min_peak=100.0) < 10
    sel, el, rank = sf.select_psf_stars(stars)
    wsel, wel, wrank = ref.select_psf_stars(stars.x, stars.y, stars.flux, stars.peak, stars.nsat,
                                            stars.status, img.shape, fwhm=4.5)
    assert same(sel, wsel) and same(el, wel) and same(rank, wrank) and len(sel) >= 6
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # a singular frame warns
        fit = pc.fit_psf(img, fwhm=4.5, **stars.psf_inputs(sel))
    assert fit.frame_status == 0 and fit.psf is not None and np.all(np.isfinite(fit.coeffs))
    print(f"{stars.n} candidates, {stars.kept.sum()} kept, {len(sel)} PSF stars, {fit.nused} used")
    import segmentation
    assert same(segmentation._positions_of(stars), np.stack([stars.x, stars.y], 1))
    pos = stars.table()[:, :2]
    got = stamps.sgp_star_stamps(img, pos, np.asarray(psf), use_betadiv=False, MAXIT=2)
    assert got["status"].shape == (len(pos),)
