"""Source detection on the device (beta-sgp_amd/segmentation.py)
against tests/golden/seg_cases.npz (astropy's convolve, scipy.ndimage's label
and measurements) and the numpy restatement tests/seg_ref.py.

Bars (derived, not measured; seg_ref.column_bars): area, boxes, min and max
exact; segment_flux 2*area*2^-53*sum|v| per segment; centroids
8*area*2^-53*max(H, W) pixels; covariances that times max(H, W).  Largest
differences measured on an MI355X, as fractions of those bars: segment_flux
0.049 against scipy (s1, s2) and 0.11 against the restatement on the
application tile; centroids 0.125 and 0.17; covariances 7e-6 and 1e-5 (also in
DESIGN §3.8).

The golden maps of s1 / s2 are stored in full, so those cases feed the golden
conv and threshold to detect_sources and the golden sub / conv / labels to
SourceCatalog and compare with scipy's columns.  The application tile's maps
are stored at every 4th row and column only: it runs end to end through
source_info with the device's own Background2D (its label images must equal
scipy's, which the generator's threshold margin guarantees), and its columns
are compared with seg_ref.catalog of the device's own sub / conv, since a
1e-14 difference between the device's and scipy's background map is larger
than the flux bar.
"""
import ctypes
import warnings

import numpy as np
import pytest

import seg_ref
from conftest import golden, ref_kwargs
from test_segmentation import check_columns, label_patterns

pytestmark = pytest.mark.gpu

CASES = ("s1", "s2")


@pytest.fixture(scope="module")
def sg():
    import _bsgp
    _bsgp.require_gpu()
    import segmentation
    return segmentation


@pytest.fixture(scope="module")
def fx():
    return seg_ref.cases()


@pytest.fixture(scope="module")
def app_tile():
    return golden("app_subdiv_inputs.npz")["img"]


def sub_of(fx, tag):
    return fx[f"{tag}_data"].astype(np.float64) - fx[f"{tag}_bkg"]


# ------------------------------------------------------------- convolution
def test_convolve_bit_equal_to_astropy(sg, fx):
    k = fx["kernel_1.2_3"]
    for tag in CASES:
        got = sg.convolve(sub_of(fx, tag), k)
        assert got.dtype == np.float64 and np.array_equal(got, fx[f"{tag}_conv"]), tag
    # the application tile (float32, widened on the device), at the stored pixels
    tile = golden("app_subdiv_inputs.npz")["img"]
    idx = fx["app_idx"]
    assert np.array_equal(sg.convolve(tile, k)[np.ix_(idx, idx)], fx["app_rawconv"])
    both = np.stack([sub_of(fx, "s1"), 2.0 * sub_of(fx, "s1")])
    got = sg.convolve(both, k)
    assert np.array_equal(got[0], fx["s1_conv"]) and np.array_equal(got[1], seg_ref.convolve(both[1], k))


def test_convolve_shapes_kernels_and_dtypes(sg, fx):
    """1 x W and H x 1 images, every kernel size, a non-square kernel, float32
    input: bit-equal to the restatement (border pixels included)."""
    rng = np.random.default_rng(5)
    for shape, ksz in (((1, 300), (3, 3)), ((70, 1), (3, 3)), ((1, 1), (7, 7)), ((33, 70), (5, 5)),
                       ((40, 257), (7, 7)), ((9, 520), (1, 7)), ((20, 20), (5, 3)), ((3, 3), (7, 7))):
        d, k = rng.normal(10.0, 3.0, shape), rng.uniform(-0.2, 1.0, ksz)
        assert np.array_equal(sg.convolve(d, k), seg_ref.convolve(d, k)), (shape, ksz)
    d32 = fx["s1_data"]
    k = fx["kernel_3.0_7"]
    a, b = sg.convolve(d32, k), sg.convolve(d32.astype(np.float64), k)
    assert np.array_equal(a, b) and np.array_equal(a, seg_ref.convolve(d32, k))
    bad = d32.astype(np.float64)
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        sg.convolve(bad, k)


def test_app_convolution_through_source_info(sg, fx, app_tile):
    """The application tile's conv at the stored pixels: the device's
    background differs from scipy's by about 1e-14 relative (DESIGN §3.7,
    |bkg| < 100), so conv agrees to 1e-11 absolute, not to the bit."""
    cat, bkg = sg.source_info(app_tile, 60)
    idx = fx["app_idx"]
    assert np.max(np.abs(cat.convolved_data[np.ix_(idx, idx)] - fx["app_conv"])) < 1e-11
    assert np.max(np.abs(bkg.background_rms[np.ix_(idx, idx)] - fx["app_rms"])) < 1e-11


# --------------------------------------------------------------- labelling
def test_labelling_patterns(sg):
    """Patterns that cross every tile border (tests/test_segmentation.py
    label_patterns), batched by (connectivity, npixels): labels equal the
    restatement's pixel for pixel."""
    groups = {}
    for name, img, conn, npix in label_patterns():
        groups.setdefault((conn, npix), []).append((name, img))
    for (conn, npix), items in groups.items():
        imgs = np.stack([i for _, i in items]).astype(np.float32)
        seg = sg.detect_sources(imgs, 0.5, npix, connectivity=conn)
        for b, (name, img) in enumerate(items):
            want, n = seg_ref.detect(img.astype(float), 0.5, npix, conn)
            assert seg.nlabels[b] == n, (name, seg.nlabels[b], n)
            np.testing.assert_array_equal(seg.data[b], want, err_msg=name)
            np.testing.assert_array_equal(seg.areas[b], np.bincount(want.ravel())[1:], err_msg=name)
            np.testing.assert_array_equal(seg.labels[b], np.arange(1, n + 1))
    # one pattern alone gives what it gives in its batch
    name, img, conn, npix = label_patterns()[0]
    alone = sg.detect_sources(img.astype(np.float64), 0.5, npix, connectivity=conn)
    np.testing.assert_array_equal(alone.data, seg_ref.detect(img.astype(float), 0.5, npix, conn)[0])
    assert alone.data.dtype == np.int32 and isinstance(alone.nlabels, int)


def test_no_detection(sg):
    z = np.zeros((150, 203))
    with pytest.warns(sg.NoDetectionsWarning):
        assert sg.detect_sources(z, 0.5, 1) is None
    one = z.copy()
    one[7, 9] = 1.0
    with pytest.warns(sg.NoDetectionsWarning):  # the only component is removed
        assert sg.detect_sources(one, 0.5, 2) is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        seg = sg.detect_sources(np.stack([z, one, z]), 0.5, 1)
    assert list(seg.nlabels) == [0, 1, 0] and not seg.data[0].any() and not seg.data[2].any()
    assert seg.data[1].sum() == 1 and seg.data[1][7, 9] == 1 and len(seg.areas[0]) == 0


def test_threshold_map_mask_and_non_finite(sg, fx):
    conv, thr = fx["s1_conv"], 1.5 * fx["s1_rms"]
    mask = np.zeros(conv.shape, bool)
    mask[20:40, 10:50] = True
    d = conv.copy()
    d[5, 5], d[6, 6], d[50, 50] = np.inf, np.nan, -np.inf
    t = thr.copy()
    t[30, 5], t[31, 6] = np.nan, -np.inf
    for kw in (dict(), dict(mask=mask)):
        seg = sg.detect_sources(d, t, 2, **kw)
        want, n = seg_ref.detect(d, t, 2, 8, kw.get("mask"))
        assert seg.nlabels == n
        np.testing.assert_array_equal(seg.data, want)
    assert not seg.data[mask].any() and seg.data[5, 5] == 0 and seg.data[31, 6] == 0
    # a scalar threshold, and one [H, W] map and mask for every image of a batch
    seg = sg.detect_sources(np.stack([conv, 2 * conv]), thr, 5, mask=mask)
    for b, c in enumerate((conv, 2 * conv)):
        np.testing.assert_array_equal(seg.data[b], seg_ref.detect(c, thr, 5, 8, mask)[0])
    np.testing.assert_array_equal(sg.detect_sources(conv, 3.0, 5).data, seg_ref.detect(conv, 3.0, 5)[0])


@pytest.mark.parametrize("tag", CASES)
def test_golden_detection_and_catalogue(sg, fx, tag):
    """Golden conv and threshold in, scipy's labels out; golden sub / conv /
    labels in, scipy's columns out within the bars."""
    sub, conv, thr = sub_of(fx, tag), fx[f"{tag}_conv"], 1.5 * fx[f"{tag}_rms"]
    for npix in (5, 1):
        seg = sg.detect_sources(conv, thr, npix)
        want = fx[f"{tag}_lab{npix}"]
        np.testing.assert_array_equal(seg.data, want)
        assert seg.nlabels == want.max()
        cat = sg.SourceCatalog(sub, seg, convolved_data=conv)
        worst = check_columns(cat.to_dict(), fx, tag, npix, sub.shape)
        print(f"{tag} n_pixels={npix}: largest difference / bar {worst}")
        np.testing.assert_array_equal(cat.label, np.arange(1, want.max() + 1))
        assert cat.segment_flux_sum == float(np.sum(cat.segment_flux))
        # a plain label image instead of the detection's object, no convolved_data
        cat2 = sg.SourceCatalog(sub, want.astype(np.int64))
        np.testing.assert_array_equal(cat2.segment_flux, cat.segment_flux)
        ref2 = seg_ref.catalog(sub, want)
        bars = seg_ref.column_bars(ref2, sub.shape)
        assert np.all(np.abs(cat2.xcentroid - ref2["xcentroid"]) <= bars["centroid"])


@pytest.mark.parametrize("tag,box", [("s1", (16, 16)), ("s2", (11, 14)), ("app", (60, 60))])
def test_source_info_end_to_end(sg, fx, app_tile, tag, box):
    """source_info with the device's own Background2D: scipy's label images
    (the generator's threshold margin), columns against the restatement on the
    device's own maps."""
    data = app_tile if tag == "app" else fx[f"{tag}_data"]
    for npix in (5, 1):
        cat, bkg = sg.source_info(data, box, n_pixels=npix)
        want = fx[f"{tag}_lab{npix}"]
        np.testing.assert_array_equal(cat.segment_img.data, want)
        assert cat.nlabels == want.max() and len(cat) == want.max()
        sub = data.astype(np.float64) - bkg.background
        assert np.array_equal(cat.data, sub)
        assert np.array_equal(cat.convolved_data, seg_ref.convolve(sub, sg.make_2dgaussian_kernel(1.2, 3)))
        ref = seg_ref.catalog(cat.data, want.astype(np.int32), cat.convolved_data)
        mine = {f"{tag}_n{npix}_{k}": v for k, v in ref.items()}
        worst = check_columns(cat.to_dict(), mine, tag, npix, sub.shape)
        print(f"{tag} n_pixels={npix} end to end: largest difference / bar {worst}")
        if tag != "app":  # scipy's columns too, up to the background's 1e-14
            np.testing.assert_allclose(cat.segment_flux, fx[f"{tag}_n{npix}_segment_flux"], rtol=1e-10)
            np.testing.assert_allclose(cat.xcentroid, fx[f"{tag}_n{npix}_xcentroid"], atol=1e-9)
        for nm in ("semimajor_sigma", "semiminor_sigma", "fwhm", "orientation"):
            assert np.all(np.isfinite(cat[nm]))
        assert np.all(cat.semimajor_sigma >= cat.semiminor_sigma)


def test_catalog_capacity_is_reported_not_overrun(sg, fx):
    """bsgp_segment_catalog with fewer rows than labels: status bits set, rows
    past cap untouched."""
    import _bsgp
    torch = _bsgp.torch
    lab = fx["s1_lab1"].astype(np.int32)
    n, cap = int(lab.max()), 3
    assert n > cap
    d = torch.from_numpy(sub_of(fx, "s1")).cuda()
    l = torch.from_numpy(lab).cuda()
    nl = torch.tensor([n], dtype=torch.int32, device="cuda")
    ic = torch.full((cap + 4, 5), -77, dtype=torch.int32, device="cuda")
    fc = torch.full((cap + 4, 8), -77.0, dtype=torch.float64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _bsgp.check(_bsgp.lib().bsgp_segment_catalog(p(d), None, p(l), 1, 64, 64, cap, p(nl), p(ic), p(fc),
                                                 p(st), _bsgp.current_stream()))
    assert int(st.cpu()[0]) == 3
    assert bool((ic[cap:] == -77).all()) and bool((fc[cap:] == -77.0).all())
    np.testing.assert_array_equal(ic[:cap, 0].cpu().numpy(), fx["s1_n1_area"][:cap])
    with pytest.raises(_bsgp.BsgpError):
        bad = lab.copy()
        bad[0, 0] = n + 5
        sg.SourceCatalog(sub_of(fx, "s1"), sg.SegmentationImage(bad, np.array([n]), False))


# ------------------------------------------------------------- determinism
def columns_equal(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def test_determinism_batch_and_dtype(sg, fx):
    s1 = fx["s1_data"]
    c1, b1 = sg.source_info(s1, 16)
    c2, b2 = sg.source_info(s1, 16)
    assert columns_equal(c1.to_dict(), c2.to_dict())
    for nm in ("data", "convolved_data"):
        assert np.array_equal(getattr(c1, nm), getattr(c2, nm))
    assert np.array_equal(c1.segment_img.data, c2.segment_img.data)
    assert np.array_equal(b1.background_rms, b2.background_rms)
    batch = np.stack([s1 + 3, s1, 2 * s1])
    cb, _ = sg.source_info(batch, 16)
    assert np.array_equal(cb.segment_img.data[1], c1.segment_img.data)
    assert columns_equal({k: v[1] for k, v in cb.to_dict().items()}, c1.to_dict())
    assert cb.segment_flux_sum[1] == c1.segment_flux_sum and list(cb.nlabels)[1] == c1.nlabels
    c64, _ = sg.source_info(s1.astype(np.float64), 16)
    assert columns_equal(c64.to_dict(), c1.to_dict())
    assert np.array_equal(c64.segment_img.data, c1.segment_img.data)
    dev, _ = sg.source_info(s1, 16, device_out=True)
    assert dev.segment_img.data.is_cuda and dev.f64_cols.is_cuda
    assert np.array_equal(dev.segment_img.data.cpu().numpy(), c1.segment_img.data)


# ------------------------------------------------------------- integration
def field96():
    """A 96 x 96 star field built like the golden s1 / s2 cases."""
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[:96, :96]
    d = 100.0 + rng.normal(0.0, 2.0, (96, 96))
    for _ in range(24):
        y0, x0, amp = rng.uniform(2, 93), rng.uniform(2, 93), rng.uniform(8.0, 60.0)
        d += amp * np.exp(-((yy - y0) ** 2 + (xx - x0) ** 2) / (2 * 1.3 ** 2))
    return d


def ref_flux_sum(sg, img, box, npix):
    """Sum of segment_flux by the restatement on the device's own background
    maps (device and restatement then see the same sub, conv and threshold),
    and the bar of that sum: the per-segment flux bars plus the rounding of
    adding n segment fluxes in two orders."""
    from background import Background2D
    b = Background2D(img, box)
    lab, n, sub, conv, _ = seg_ref.source_info(img, b.background, b.background_rms, n_pixels=npix,
                                               kernel=sg.make_2dgaussian_kernel(1.2, 3))
    cat = seg_ref.catalog(sub, lab, conv)
    bar = seg_ref.column_bars(cat, img.shape)["flux"].sum() + \
        2 * n * 2.0 ** -53 * np.abs(cat["segment_flux"]).sum()
    return float(cat["segment_flux"].sum()), float(bar)


def solve_kwargs():
    fx64 = golden("ref_lin64_beta.npz")
    kw = ref_kwargs(fx64)
    kw.update(MAXIT=5, verbose=False)
    return fx64["psf"], kw


def test_subdivisions_flux_from_segments(sg, monkeypatch, tmp_path):
    import sgp
    import subdivisions
    monkeypatch.chdir(tmp_path)
    psf, kw = solve_kwargs()
    beta = kw.pop("betaParam")
    field = field96()
    seen = {}
    real = sgp.sgp_betaDiv_batch

    def spy(gns, *a, **k):
        seen["flux"], seen["gns"] = np.asarray(k["flux"]), gns.cpu().numpy()
        return real(gns, *a, **k)

    monkeypatch.setattr(sgp, "sgp_betaDiv_batch", spy)
    mosaic, foot, out = subdivisions.sgp_subdivisions(
        field, psf, "estimate", subdiv_shape=(64, 64), overlap=32, betaParams=beta,
        bkg_box_size=16, flux="segments", **kw)
    boxes = subdivisions.subdivision_boxes((96, 96), (64, 64), 32)
    assert seen["flux"].shape == (len(boxes),) and len(boxes) == 4 and mosaic.shape == (96, 96)
    for t, (x0, y0, x1, y1) in enumerate(boxes):
        tile = field[y0:y1, x0:x1]
        assert np.array_equal(seen["gns"][t], tile)
        want, bar = ref_flux_sum(sg, tile, 16, 5)
        assert want > 0 and abs(seen["flux"][t] - want) <= bar, (t, seen["flux"][t], want, bar)
    assert np.all(np.isfinite(mosaic)) and np.all(foot >= 1)
    with pytest.raises(ValueError, match="bkg_box_size"):
        subdivisions.sgp_subdivisions(field, psf, 100.0, subdiv_shape=(64, 64), overlap=32,
                                      betaParams=beta, flux="segments", **kw)


def test_multistart_scores_with_flux_fraction(sg, fx, monkeypatch, tmp_path):
    import sgp
    monkeypatch.chdir(tmp_path)
    psf, kw = solve_kwargs()
    kw.pop("betaParam")
    gn = fx["s1_data"].astype(np.float64)
    betas = [1.02, 1.3, 1.6]
    score = sg.flux_fraction_score(gn, box_size=16)
    (x, it, discr, _, _), info = sgp.sgp_betaDiv_multistart(
        gn, psf, np.float64(100.0), betas=betas, score=score, final_solve=False, **kw)
    den, dbar = ref_flux_sum(sg, gn, 16, 5)
    xs = np.stack([c[0] for c in info["candidates"]])
    for i, c in enumerate(xs):
        num, nbar = ref_flux_sum(sg, c, 16, 1)
        want = 1.0 - num / den
        bar = (nbar + abs(num / den) * dbar) / abs(den) + 4 * 2.0 ** -53 * (1 + abs(num / den))
        assert abs(info["scores"][i] - want) <= bar, (i, info["scores"][i], want, bar)
        assert score(c) == info["scores"][i]  # .batch and one call at a time: the same bits
    assert list(score.batch(xs)) == info["scores"]
    assert info["best"] == sgp.argmin_strict(info["scores"]) and np.array_equal(x, xs[info["best"]])
    # a plain callable is used as before
    _, plain = sgp.sgp_betaDiv_multistart(gn, psf, np.float64(100.0), betas=betas,
                                          score=lambda x: -float(np.max(x)), final_solve=False, **kw)
    assert plain["scores"] == [-float(np.max(c[0])) for c in plain["candidates"]]
