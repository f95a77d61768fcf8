"""Source detection, the checks that need no device: the kernel against
astropy's, the numpy restatement tests/seg_ref.py against
tests/golden/seg_cases.npz (astropy's convolve, scipy.ndimage's label and
measurements; tests/golden/make_golden_seg.py), the host shape formulas, and
the argument errors of segmentation.py and of the three C entry points, which
are raised before any device work."""
import ctypes
import inspect

import numpy as np
import pytest

import seg_ref

CASES = ("s1", "s2")
INT_COLS = ("area", "bbox_xmin", "bbox_xmax", "bbox_ymin", "bbox_ymax")
EXACT_COLS = INT_COLS + ("min_value", "max_value")


@pytest.fixture(scope="module")
def fx():
    return seg_ref.cases()


def check_columns(got, fx, tag, npix, shape, record=None):
    """Catalogue columns against the golden ones of case tag / npixels: area,
    boxes, min and max exact; flux, centroids and covariances within the
    derived bars (seg_ref.column_bars).  Returns the largest differences."""
    pre = f"{tag}_n{npix}_"
    want = {k[len(pre):]: v for k, v in fx.items() if k.startswith(pre)}
    bars = seg_ref.column_bars(want, shape)
    for k in EXACT_COLS:
        np.testing.assert_array_equal(np.asarray(got[k]), want[k], err_msg=f"{tag} {k}")
    worst = {}
    for k, bar in (("segment_flux", bars["flux"]), ("xcentroid", bars["centroid"]),
                   ("ycentroid", bars["centroid"]), ("covar_sigx2", bars["covar"]),
                   ("covar_sigxy", bars["covar"]), ("covar_sigy2", bars["covar"])):
        diff = np.abs(np.asarray(got[k]) - want[k])
        worst[k] = float(np.max(diff / bar))
        assert np.all(diff <= bar), (tag, npix, k, float(diff.max()), float(bar.min()))
    if record is not None:
        record[(tag, npix)] = worst
    return worst


def test_golden_cases_are_what_they_claim(fx):
    assert fx["app_nraw"] == 459 and fx["app_lab1"].max() == 459 and fx["app_lab5"].max() == 93
    assert fx["app_largest"] == 511
    for tag in ("app",) + CASES:
        assert float(fx[f"{tag}_margin"]) >= 1e-9, tag
        assert 0 < fx[f"{tag}_lab5"].max() < fx[f"{tag}_lab1"].max() == fx[f"{tag}_nraw"], tag
    assert float(fx["app_margin"]) > 5e-5  # measured 5.8e-5
    assert fx["s1_data"].shape == (64, 64) and fx["s2_data"].shape == (33, 70)
    assert fx["s1_data"].dtype == np.float32


def test_kernel_matches_astropy(fx):
    from segmentation import make_2dgaussian_kernel
    assert len(fx["kernel_list"]) == 3
    for fwhm, size in fx["kernel_list"]:
        want = fx[f"kernel_{fwhm}_{int(size)}"]
        for got in (make_2dgaussian_kernel(fwhm, int(size)), seg_ref.make_kernel(fwhm, int(size))):
            assert got.shape == want.shape
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    k = make_2dgaussian_kernel(1.2, 3)
    np.testing.assert_allclose(k[0, :2], [0.02617386, 0.10943565], rtol=2e-7)
    assert abs(k.sum() - 1) < 1e-15
    assert np.allclose(k, k.T, rtol=1e-14, atol=0) and np.allclose(k, k[::-1], rtol=1e-14, atol=0)


@pytest.mark.parametrize("tag", CASES)
def test_restatement_matches_golden(fx, tag):
    """seg_ref against astropy / scipy: conv bit-equal, labels equal, columns
    within the derived bars."""
    d, bkg, rms = fx[f"{tag}_data"], fx[f"{tag}_bkg"], fx[f"{tag}_rms"]
    for npix in (5, 1):
        lab, n, sub, conv, _ = seg_ref.source_info(d, bkg, rms, n_pixels=npix,
                                                   kernel=fx["kernel_1.2_3"])
        assert np.array_equal(conv, fx[f"{tag}_conv"])  # to the last bit
        np.testing.assert_array_equal(lab, fx[f"{tag}_lab{npix}"])
        assert n == fx[f"{tag}_lab{npix}"].max()
        check_columns(seg_ref.catalog(sub, lab, conv), fx, tag, npix, d.shape)


def test_restatement_convolves_the_application_tile_bit_equal(fx):
    from conftest import golden
    tile, idx = golden("app_subdiv_inputs.npz")["img"], fx["app_idx"]
    got = seg_ref.convolve(tile, fx["kernel_1.2_3"])
    assert np.array_equal(got[np.ix_(idx, idx)], fx["app_rawconv"])


def test_restatement_convolution_borders():
    """The zero fill at the border and degenerate shapes, against the
    definition written out per pixel."""
    rng = np.random.default_rng(3)
    for shape, ksz in (((1, 9), (3, 3)), ((7, 1), (3, 5)), ((6, 5), (7, 7))):
        d, k = rng.normal(size=shape), rng.uniform(0.1, 1.0, ksz)
        got = seg_ref.convolve(d, k)
        kh, kw = ksz
        for y in range(shape[0]):
            for x in range(shape[1]):
                acc = 0.0
                for i in range(kh):
                    for j in range(kw):
                        yy, xx = y + i - kh // 2, x + j - kw // 2
                        v = d[yy, xx] if 0 <= yy < shape[0] and 0 <= xx < shape[1] else 0.0
                        acc = acc + v * k[kh - 1 - i, kw - 1 - j]
                assert got[y, x] == acc / k.sum()


def label_patterns(H=150, W=203):
    """0/1 images that stress a tiled labeller: (name, image, connectivity,
    npixels).  150 x 203 is no multiple of 16, 32 or 64 and spans at least
    three tiles of 64 per axis."""
    out = []
    sp = np.zeros((H, W), np.uint8)  # one-pixel-wide spiral, one empty pixel between its turns
    y = x = 0
    dy, dx = 0, 1
    sp[0, 0] = 1
    turns = 0
    while turns < 2:
        ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < H and 0 <= nx < W and not sp[ny, nx] and \
                not (0 <= my < H and 0 <= mx < W and sp[my, mx]):
            y, x, turns = ny, nx, 0
            sp[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1
    out.append(("spiral", sp, 8, 1))
    out.append(("spiral4", sp, 4, 1))
    se = np.zeros((H, W), np.uint8)  # serpentine: rows 0, 2, 4.. joined at alternating ends
    se[::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        se[y, W - 1 if k % 2 == 0 else 0] = 1
    out.append(("serpentine", se, 4, 1))
    sv = se[:, :H].T.copy()  # the same, column-wise
    out.append(("serpentine_cols", np.pad(sv, ((0, 0), (0, W - sv.shape[1]))), 8, 1))
    u = np.zeros((H, W), np.uint8)  # arms meet only in the last rows; a blob between them
    u[5:, 10] = 1
    u[2:, 190] = 1
    u[H - 1, 10:191] = 1
    u[3:9, 90:100] = 1
    u[0, 200] = 1
    out.append(("u", u, 8, 1))
    cb = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.uint8)
    out.append(("checker8", cb, 8, 1))
    out.append(("checker4", cb, 4, 1))
    for c in range(16, min(H, W) - 3, 16):  # two blocks touching only diagonally at (c, c)
        dg = np.zeros((H, W), np.uint8)
        dg[c - 3:c, c - 3:c] = 1
        dg[c:c + 3, c:c + 3] = 1
        dg[c - 3:c, c + 40:c + 43] = 1  # and an anti-diagonal pair
        dg[c:c + 3, c + 37:c + 40] = 1
        out.append((f"diag{c}_8", dg, 8, 1))
        out.append((f"diag{c}_4", dg, 4, 1))
    out.append(("all_true", np.ones((H, W), np.uint8), 8, 1))
    co = np.zeros((H, W), np.uint8)
    co[0, 0] = co[0, -1] = co[-1, 0] = co[-1, -1] = 1
    out.append(("corners", co, 8, 1))
    rng = np.random.default_rng(11)
    rn = (rng.random((H, W)) < 0.42).astype(np.uint8)
    out.append(("random_np1", rn, 4, 1))
    out.append(("random_np4", rn, 4, 4))  # survivors renumbered consecutively
    out.append(("random8_np30", rn, 8, 30))
    return out


def test_labeller_matches_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, img, conn, _ in label_patterns():
        st = np.ones((3, 3), int) if conn == 8 else None
        want, n = ndimage.label(img, structure=st)
        got, m = seg_ref.label(img, conn)
        assert m == n, name
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_patterns_exercise_what_they_claim():
    pats = {n: (i, c, p) for n, i, c, p in label_patterns()}
    assert seg_ref.label(pats["spiral"][0], 8)[1] == 1
    assert seg_ref.label(pats["serpentine"][0], 4)[1] == 1
    lab, n = seg_ref.label(pats["u"][0], 8)
    assert n == 3 and lab[2, 190] == 2 and lab[5, 10] == 2 and lab[3, 90] == 3 and lab[0, 200] == 1
    assert seg_ref.label(pats["checker8"][0], 8)[1] == 1
    assert seg_ref.label(pats["checker4"][0], 4)[1] == pats["checker4"][0].sum()
    assert seg_ref.label(pats["diag64_8"][0], 8)[1] == 2 and seg_ref.label(pats["diag64_4"][0], 4)[1] == 4
    img = pats["random_np4"][0]
    lab, n = seg_ref.detect(img.astype(float), 0.5, 4, 4)
    assert 0 < n < seg_ref.label(img, 4)[1] and set(np.unique(lab)) == set(range(n + 1))


def test_shape_formulas_on_an_elliptical_gaussian():
    """An elliptical Gaussian (sigmas 3 and 1.5, rotated by 30 degrees) sampled
    finely over +-8 sigma: its weighted covariance gives back its parameters."""
    from segmentation import shape_columns
    a, b, th = 3.0, 1.5, np.radians(30.0)
    yy, xx = np.mgrid[-40:41, -40:41] * 0.5
    u, v = xx * np.cos(th) + yy * np.sin(th), -xx * np.sin(th) + yy * np.cos(th)
    w = np.exp(-0.5 * ((u / a) ** 2 + (v / b) ** 2))
    s = w.sum()
    sx2, sxy, sy2 = (w * xx * xx).sum() / s, (w * xx * yy).sum() / s, (w * yy * yy).sum() / s
    c = shape_columns([sx2], [sxy], [sy2])
    assert abs(c["semimajor_sigma"][0] - a) < 1e-6 and abs(c["semiminor_sigma"][0] - b) < 1e-6
    assert abs(c["orientation"][0] - 30.0) < 1e-6
    assert abs(c["eccentricity"][0] - np.sqrt(1 - (b / a) ** 2)) < 1e-6
    assert abs(c["ellipticity"][0] - 0.5) < 1e-6
    assert abs(c["fwhm"][0] - 2 * np.sqrt(np.log(2) * (a * a + b * b))) < 1e-5
    r = shape_columns([2.0], [0.0], [2.0])  # a circle
    assert r["eccentricity"][0] == 0 and r["ellipticity"][0] == 0
    assert abs(r["fwhm"][0] - 2 * np.sqrt(2 * np.log(2)) * np.sqrt(2.0)) < 1e-14


def test_argument_errors_need_no_device():
    import segmentation as sg
    img = np.ones((21, 21))
    for bad in (np.ones((2, 2)), np.ones((3, 4)), np.ones((9, 9)), np.ones((3, 9)), np.ones(3)):
        with pytest.raises(ValueError, match="kernel"):
            sg.convolve(img, bad)
    with pytest.raises(ValueError, match="size"):
        sg.make_2dgaussian_kernel(1.2, 4)
    with pytest.raises(ValueError, match="fwhm"):
        sg.make_2dgaussian_kernel(0.0, 3)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="npixels"):
            sg.detect_sources(img, 0.5, bad)
    for bad in (6, 0, 1):
        with pytest.raises(ValueError, match="connectivity"):
            sg.detect_sources(img, 0.5, 5, connectivity=bad)
    with pytest.raises(ValueError, match="threshold shape"):
        sg.detect_sources(img, np.ones((21, 20)), 5)
    with pytest.raises(ValueError, match="mask shape"):
        sg.detect_sources(np.ones((2, 21, 21)), 0.5, 5, mask=np.zeros((3, 21, 21), bool))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        sg.detect_sources(np.ones(21), 0.5, 5)
    with pytest.raises(ValueError, match="segment_img shape"):
        sg.SourceCatalog(img, np.zeros((21, 20), np.int32))
    with pytest.raises(ValueError, match="convolved_data shape"):
        sg.SourceCatalog(img, np.zeros((21, 21), np.int32), convolved_data=np.ones((20, 21)))
    with pytest.raises(ValueError, match="npixels"):
        sg.source_info(img, 7, n_pixels=0)
    s = inspect.signature(sg.source_info)
    assert list(s.parameters)[:4] == ["data", "box_size", "n_pixels", "sigma_threshold"]
    assert s.parameters["n_pixels"].default == 5 and s.parameters["sigma_threshold"].default == 1.5
    s = inspect.signature(sg.flux_fraction_score)
    assert [(k, p.default) for k, p in s.parameters.items()][1:] == \
        [("box_size", 60), ("n_pixels_orig", 5), ("n_pixels_restored", 1), ("sigma_threshold", 1.5)]
    assert hasattr(sg.flux_fraction_score(img), "batch")


def test_unknown_and_unavailable_columns():
    import segmentation as sg
    cat = sg.SourceCatalog.__new__(sg.SourceCatalog)
    cat._cols, cat.batched = {"label": [np.arange(1, 3)]}, False
    assert list(cat["label"]) == [1, 2] and list(cat.label) == [1, 2]
    for name, word in (("sky_centroid", "WCS"), ("local_background", "background"),
                       ("segment_fluxerr", "error")):
        with pytest.raises(KeyError, match=word):
            cat[name]
        with pytest.raises(KeyError, match=word):
            cat.to_dict(["label", name])
    with pytest.raises(KeyError, match="unknown column"):
        cat["kron_flux"]
    with pytest.raises(AttributeError):
        cat.kron_flux
    assert set(sg.INT_COLUMNS + sg.F64_COLUMNS + sg.SHAPE_COLUMNS) < set(sg.COLUMNS)


def test_no_cpu_fallback():
    import _bsgp
    import segmentation as sg
    if _bsgp.torch is not None and _bsgp.torch.cuda.is_available():
        return  # tests/test_gpu_segmentation.py runs it
    img = np.ones((21, 21))
    for call in (lambda: sg.convolve(img, np.ones((3, 3))), lambda: sg.detect_sources(img, 0.5, 1),
                 lambda: sg.SourceCatalog(img, np.ones((21, 21), np.int32)),
                 lambda: sg.source_info(img, 7)):
        with pytest.raises(_bsgp.BsgpError):
            call()


def test_c_abi_argument_errors():
    """The three entry points validate on the host before any device call:
    BSGP_ERR_ARG names the field, the kernel and size limits are
    BSGP_ERR_UNSUPPORTED and name the limit."""
    import _bsgp
    L = _bsgp.lib()
    for name in ("bsgp_convolve2d", "bsgp_detect_sources", "bsgp_segment_catalog"):
        assert name in _bsgp.EXPORTED and hasattr(L, name)
    assert L.bsgp_abi_version() == 3
    buf = np.zeros((64, 64))
    p = ctypes.c_void_p(buf.ctypes.data)  # never dereferenced: every call below fails validation

    def conv(data=p, dtype=1, B=1, H=64, W=64, kernel=p, kh=3, kw=3, out=p):
        rc = L.bsgp_convolve2d(data, dtype, B, H, W, kernel, kh, kw, out, None)
        return rc, L.bsgp_last_error().decode()

    def det(data=p, dtype=1, B=1, H=64, W=64, npixels=5, conn=8, lab=p, n=p):
        rc = L.bsgp_detect_sources(data, dtype, B, H, W, None, 0.5, npixels, conn, None, lab, n, None)
        return rc, L.bsgp_last_error().decode()

    def cat(data=p, labels=p, B=1, H=64, W=64, cap=4, ic=p, fc=p, st=p):
        rc = L.bsgp_segment_catalog(data, None, labels, B, H, W, cap, None, ic, fc, st, None)
        return rc, L.bsgp_last_error().decode()

    for fn, kw, word in ((conv, dict(data=None), "data"), (conv, dict(kernel=None), "kernel"),
                         (conv, dict(out=None), "out"), (conv, dict(dtype=2), "dtype"),
                         (conv, dict(B=0), "B"), (conv, dict(kh=0), "kernel size"),
                         (det, dict(data=None), "data"), (det, dict(lab=None), "labels_out"),
                         (det, dict(n=None), "nlabels_out"), (det, dict(dtype=-1), "dtype"),
                         (det, dict(npixels=0), "npixels"), (det, dict(conn=6), "connectivity"),
                         (det, dict(W=0), "W"),
                         (cat, dict(data=None), "data"), (cat, dict(labels=None), "labels"),
                         (cat, dict(cap=0), "cap"), (cat, dict(st=None), "status_out"),
                         (cat, dict(H=-1), "H")):
        rc, msg = fn(**kw)
        assert rc == _bsgp.BSGP_ERR_ARG and word in msg, (fn.__name__, kw, rc, msg)
    for kw in (dict(kh=4), dict(kw=2), dict(kh=9), dict(kw=9)):
        rc, msg = conv(**kw)
        assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and "7 x 7" in msg, (kw, rc, msg)
    for fn in (conv, det, cat):
        rc, msg = fn(H=65536, W=32768)
        assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and "2^31" in msg, (fn.__name__, rc, msg)


def test_multistart_and_subdivisions_accept_the_new_values():
    import subdivisions
    for fn in (subdivisions.sgp_subdivisions, subdivisions.sgp_subdivisions_multistart):
        with pytest.raises(ValueError, match="bkg_box_size"):
            subdivisions._segment_flux({"flux": "segments"}, None, None)
        with pytest.raises(ValueError, match="segments"):
            subdivisions._segment_flux({"flux": "sources"}, None, 16)
        assert "segments" in fn.__doc__
    kw = {"flux": 3.5}
    subdivisions._segment_flux(kw, None, None)  # any other flux is passed through
    assert kw == {"flux": 3.5}
    kw = {}
    subdivisions._segment_flux(kw, None, None)
    assert kw == {}
