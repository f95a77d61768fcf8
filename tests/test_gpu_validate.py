"""Source validation on the device (``bsgp_validate_sources``,
``segmentation.validate_sources`` / ``validation_source`` /
``source_info(validate=True)``) against the numpy
restatement tests/validate_ref.py: the statistics bit for bit
(``np.array_equal(..., equal_nan=True)``: the sign of a zero is not
distinguished), ``valid`` and ``status`` exactly."""
import numpy as np
import pytest

import _bsgp
import segmentation as sg
import seg_ref
from segmentation import validate_sources, validation_source
from validate_ref import validate_one, validate_ref

pytestmark = pytest.mark.gpu

H, W = 160, 144
PARTIAL, NO_OVERLAP, BAD = (_bsgp.BSGP_STAMP_PARTIAL, _bsgp.BSGP_STAMP_NO_OVERLAP,
                            _bsgp.BSGP_STAMP_BAD_POSITION)


def frames(seed=0, dtype=np.float64):
    """(image, bkgmap, rmsmap) of H x W: values that round at every addition."""
    rng = np.random.default_rng(seed)
    img = (100.0 + rng.normal(0.0, 3.0, (H, W)) + 40.0 * (rng.random((H, W)) > 0.995)).astype(dtype)
    bkg = 100.0 + rng.normal(0.0, 0.7, (H, W))
    rms = np.abs(rng.normal(3.0, 0.4, (H, W)))
    return img, bkg, rms


def check(res, ref, what=""):
    stats = np.stack([res.source_pixs, res.bkg, res.rms], axis=1) if len(res.valid) else \
        np.zeros((0, 3))
    assert np.array_equal(stats, ref["stats"], equal_nan=True), \
        (what, np.argwhere(~((stats == ref["stats"]) | (np.isnan(stats) & np.isnan(ref["stats"])))))
    assert np.array_equal(res.valid, ref["valid"]) and res.valid.dtype == bool, what
    assert np.array_equal(res.status, ref["status"]), what


def both(img, pos, bkg, rms, size, nsigma=3.0):
    res = validate_sources(img, pos, bkg, rms, size=size, nsigma=nsigma)
    ref = validate_ref(img, pos, bkg, rms, size, nsigma)
    check(res, ref, f"size {size}")
    return res, ref


@pytest.fixture(scope="module")
def f64():
    return frames(0)


@pytest.fixture(scope="module")
def positions():
    rng = np.random.default_rng(5)
    return np.stack([rng.uniform(-3.0, W + 3.0, 40), rng.uniform(-3.0, H + 3.0, 40)], axis=1)


# 1 ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("size", [1, 2, 7, 12, (9, 14), 100, 128])
def test_sizes_that_split_the_code_paths(f64, positions, size):
    img, bkg, rms = f64
    res, ref = both(img, positions, bkg, rms, size)
    assert np.isfinite(ref["stats"][ref["status"] <= PARTIAL]).all()


def test_size_over_the_cap_raises(f64, positions):
    with pytest.raises(ValueError, match="VALIDATE_MAX"):
        validate_sources(f64[0], positions, f64[1], f64[2], size=129)


# 2 ------------------------------------------------------------------ box rule and edges
@pytest.mark.parametrize("size", [7, 12])
def test_box_rule_and_edges(f64, size):
    img, bkg, rms = f64
    pos = [(0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0),      # corners
           (-0.5, 80.0), (W - 0.5, 80.0), (70.0, -0.5), (70.0, H - 0.5),        # half outside
           (50.0, 60.0), (50.5, 60.5), (51.0, 60.5), (50.5, 61.0),              # k and k + 0.5
           (np.nextafter(50.5, 0.0), 60.0), (np.nextafter(50.5, 99.0), 60.0),
           (1e6, 50.0), (-1e12, -1e12), (70.0, H + size), (70.0, -size - 1.0),  # no overlap
           (np.nan, 50.0), (50.0, np.inf), (-np.inf, np.nan)]                   # bad positions
    res, ref = both(img, pos, bkg, rms, size)
    assert ref["status"][:8].tolist() == [PARTIAL] * 8
    assert ref["status"][8:14].tolist() == [0] * 6
    assert ref["status"][14:18].tolist() == [NO_OVERLAP] * 4
    assert ref["status"][18:].tolist() == [BAD] * 3
    assert np.isnan(res.source_pixs[14:]).all() and not res.valid[14:].any()
    # k vs k + 0.5 move the box by a pixel for one parity of the size only
    assert (ref["stats"][8, 2] != ref["stats"][9, 2]) == (size % 2 == 0)
    assert (ref["stats"][12, 2] != ref["stats"][13, 2]) == (size % 2 == 1)


def test_corner_window_mostly_fill(f64):
    """More than half of the cells lie in the fill region: the median is the fill."""
    img, bkg, rms = f64
    res, ref = both(img, [(-2.0, -2.0), (W + 1.0, H + 1.0)], bkg, rms, 12)
    assert ref["stats"][:, 1].tolist() == [0.0, 0.0] and ref["status"].tolist() == [PARTIAL] * 2
    assert (ref["stats"][:, 0] > 0).all()


# 3 ------------------------------------------------------------------ ties
@pytest.mark.parametrize("size", [7, 12, 100])
def test_ties_negative_values_and_zeros(positions, size):
    rng = np.random.default_rng(9)
    levels = np.array([-2.0, -0.0, 0.0, 1.0, 3.0])
    img = levels[rng.integers(0, 5, (H, W))]
    bkg = levels[rng.integers(0, 5, (H, W))]
    rms = levels[rng.integers(2, 5, (H, W))]
    res, ref = both(img, positions, bkg, rms, size)
    seen = ref["stats"][ref["status"] <= PARTIAL, 1]  # medians out of large equal buckets
    assert np.isin(seen, np.concatenate([levels, [0.5, -1.0, 2.0]])).all()
    res, ref = both(-np.abs(img) - 1.0, positions, -bkg, rms, size)  # all image values negative
    assert (ref["stats"][:, 0] < 0).any()


def test_even_window_with_two_different_middle_values(f64):
    img, _, rms = f64
    bkg = np.zeros((H, W))
    bkg[60:62, 50:52] = [[1.0, 2.0], [4.0, 50.0]]
    res, ref = both(img, [(51.0, 61.0)], bkg, rms, 2)
    assert ref["stats"][0, 1] == 3.0  # (2 + 4) / 2, not a value of the window
    bkg = np.arange(H * W, dtype=np.float64).reshape(H, W) * 0.1
    res, ref = both(img, [(51.0, 61.0), (80.3, 20.9)], bkg, rms, 12)
    win = bkg[55:67, 45:57]
    assert ref["stats"][0, 1] not in win


# 4 ------------------------------------------------------------------ non-finite pixels
def test_non_finite_pixels(f64):
    img, bkg, rms = (a.copy() for a in f64)
    pos = [(20.0, 20.0), (60.0, 20.0), (100.0, 20.0), (20.0, 100.0), (60.0, 100.0), (100.0, 100.0)]
    img[20, 21] = np.nan
    bkg[22, 60] = np.nan
    rms[19, 100] = np.nan
    img[100, 20] = np.inf
    bkg[101, 61] = -np.inf   # sorts first: the median stays finite
    rms[99, 99] = np.inf
    res, ref = both(img, pos, bkg, rms, 12)
    assert np.isnan(ref["stats"][0, 0]) and np.isfinite(ref["stats"][0, 1:]).all()
    assert np.isnan(ref["stats"][1, 1]) and np.isnan(ref["stats"][2, 2])
    assert ref["stats"][3, 0] == np.inf and ref["valid"][3]
    assert np.isfinite(ref["stats"][4, 1])
    assert ref["stats"][5, 2] == np.inf and not ref["valid"][5]
    assert not ref["valid"][:3].any()
    both(img, pos, bkg, rms, 100)  # every window now holds several of them


# 5 ------------------------------------------------------------------ float32 image
def test_float32_image_in_float32_arithmetic(positions):
    img, bkg, rms = frames(3, np.float32)
    rng = np.random.default_rng(17)
    while True:  # three top values whose float32 sum rounds differently from the float64 one
        top = np.sort(rng.uniform(200.0, 300.0, 3).astype(np.float32))
        if np.float64(top.mean()) != top.astype(np.float64).mean():
            break
    assert top.mean().dtype == np.float32
    img[70, 60], img[72, 63], img[69, 58] = top
    pos = np.concatenate([positions, [(60.0, 70.0)]])
    for size in (7, 12, 100):
        res, ref = both(img, pos, bkg, rms, size)
        assert ref["stats"][-1, 0] == np.float64(top.mean())
        r64 = validate_ref(img.astype(np.float64), pos, bkg, rms, size)
        assert ref["stats"][-1, 0] != r64["stats"][-1, 0]
        assert np.array_equal(ref["stats"][:, 1:], r64["stats"][:, 1:], equal_nan=True)


# 6 ------------------------------------------------------------------ verdict boundary
def test_verdict_boundary_is_strict():
    img = np.ones((H, W))
    bkg, rms = np.full((H, W), 1.0), np.full((H, W), 0.5)
    img[40, 40] = img[41, 42] = img[38, 39] = 2.5
    img[100, 100] = img[101, 102] = img[98, 99] = np.nextafter(2.5, 3.0)
    res, ref = both(img, [(40.0, 40.0), (100.0, 100.0)], bkg, rms, 7)
    assert ref["stats"][0].tolist() == [2.5, 1.0, 0.5]  # 2.5 > 1.0 + 3 * 0.5 is false
    assert ref["valid"].tolist() == [False, True] and res.valid.tolist() == [False, True]
    res, ref = both(img, [(40.0, 40.0), (100.0, 100.0)], bkg, rms, 7, nsigma=2.5)
    assert res.valid.tolist() == [True, True]


# 7 ------------------------------------------------------------------ batch
def test_batch_shared_and_per_image_maps(positions):
    torch = _bsgp.torch
    fr = [frames(s) for s in (11, 12, 13)]
    imgs = np.stack([f[0] for f in fr])
    bkgs, rmss = np.stack([f[1] for f in fr]), np.stack([f[2] for f in fr])
    pos = [np.zeros((0, 2)), positions[:5], positions[5:22]]
    for size in (7, 100):
        for maps in ((bkgs[0], rmss[0]), (bkgs, rmss)):
            res = validate_sources(imgs, pos, *maps, size=size)
            dev = validate_sources(imgs, pos, *maps, size=size, device_out=True)
            assert [len(v) for v in res.valid] == [0, 5, 17]
            for b in range(3):
                bm, rm = (m if m.ndim == 2 else m[b] for m in maps)
                one = validate_sources(imgs[b], pos[b], bm, rm, size=size)
                check(one, validate_ref(imgs[b], pos[b], bm, rm, size), f"image {b}")
                for k in ("valid", "source_pixs", "bkg", "rms", "status"):
                    got, d = getattr(res, k)[b], getattr(dev, k)[b]
                    assert np.array_equal(got, getattr(one, k), equal_nan=True), (k, b)
                    assert torch.is_tensor(d) and d.is_cuda
                    assert np.array_equal(d.cpu().numpy(), got, equal_nan=True), (k, b)
            assert dev.stats_dev.shape == (3, 17, 3) and dev.valid_dev.is_cuda
            assert dev.valid[2].dtype == torch.bool


# 8 ------------------------------------------------------------------ validation_source
def test_validation_source_is_the_one_row_call(f64, positions):
    img, bkg, rms = f64
    seen = set()
    for p in positions[:12]:
        v = validation_source(img, tuple(p), bkg, rms, size=7)
        assert type(v) is bool
        assert v == bool(validate_sources(img, p[None], bkg, rms, size=7).valid[0])
        assert v == validate_one(img, p, bkg, rms, 7)[0]
        seen.add(v)
    assert seen == {True, False}
    assert validation_source(img, (70.0, 80.0), bkg, rms) == validate_one(img, (70.0, 80.0), bkg, rms)[0]
    assert validation_source(img, (np.nan, 80.0), bkg, rms) is False


# 9 ------------------------------------------------------------------ source_info(validate=True)
FIELD_SIGMA = 2.0  # rms of the field's uniform noise


def restored_like_field():
    """A 128 x 128 restored-like field: a flat sky of 100 with uniform noise of
    rms FIELD_SIGMA (so no noise pixel exceeds sqrt(3) sigma), six Gaussian
    stars of 60 to 200 sigma and eight planted single pixels of exactly 4.5
    sigma, each at least 12 pixels from every star and from each other."""
    rng = np.random.default_rng(21)
    a = FIELD_SIGMA * np.sqrt(3.0)
    d = 100.0 + rng.uniform(-a, a, (128, 128))
    yy, xx = np.mgrid[:128, :128]
    stars = [(20.3, 24.8), (30.1, 100.6), (64.5, 60.2), (100.9, 20.4), (104.2, 104.7), (70.0, 112.5)]
    for k, (y0, x0) in enumerate(stars):
        d += FIELD_SIGMA * (60.0 + 28.0 * k) * np.exp(-((yy - y0) ** 2 + (xx - x0) ** 2) / (2 * 1.3 ** 2))
    faint = [(12, 60), (40, 40), (45, 80), (60, 20), (85, 50), (88, 84), (115, 62), (50, 118)]
    for y, x in faint:
        d[y, x] = 100.0 + 4.5 * FIELD_SIGMA
    return d, stars, faint


def test_source_info_validate():
    """source_info(validate=True) on the restored-like field with n_pixels=1:
    ``valid`` equals validate_sources on the host copies of the same catalogue
    and the restatement at those centroids, on the device's own maps.  The
    field is built so that both verdicts occur: with a 9 x 9 window a star's
    three top pixels stand tens of sigma over the sky, while a planted pixel of
    4.5 sigma and two noise pixels of at most sqrt(3) sigma average less than 3
    sigma.  That was checked on the CPU with the restatements (seg_ref's
    detection on constant maps of 100 and FIELD_SIGMA, validate_ref at the
    detections' centroids: 6 valid stars, 8 invalid planted pixels) and is
    asserted below on the restatement with the device's maps."""
    field, stars, faint = restored_like_field()
    cat, bkg = sg.source_info(field, 32, n_pixels=1, validate=True, validate_size=9)
    plain, _ = sg.source_info(field, 32, n_pixels=1)
    # validate=False: no `valid`, otherwise the same catalogue
    assert "valid" not in plain.to_dict() and not hasattr(plain, "validation")
    assert not hasattr(plain, "segment_flux_sum_valid")
    with pytest.raises(KeyError):
        plain["valid"]
    dv = cat.to_dict()
    assert list(dv)[-1] == "valid" and dv["valid"].dtype == bool and len(dv["valid"]) == cat.nlabels
    for k, v in plain.to_dict().items():
        assert np.array_equal(v, dv[k], equal_nan=True), k
    assert np.array_equal(plain.segment_img.data, cat.segment_img.data)
    assert plain.segment_flux_sum == cat.segment_flux_sum
    # against validate_sources on the host columns and the restatement
    pos = np.stack([cat.xcentroid, cat.ycentroid], axis=1)
    host = validate_sources(field, pos, bkg.background, bkg.background_rms, size=9)
    ref = validate_ref(field, pos, bkg.background, bkg.background_rms, 9)
    check(host, ref)
    check(cat.validation, ref)
    assert np.array_equal(cat.valid, ref["valid"])
    assert np.array_equal(validate_sources(field, cat, bkg.background, bkg.background_rms, size=9).valid,
                          cat.valid)
    # both verdicts, at the sources they were built for
    lab = cat.segment_img.data
    star_rows = [lab[int(round(y)), int(round(x))] - 1 for y, x in stars]
    faint_rows = [lab[y, x] - 1 for y, x in faint]
    assert min(star_rows) >= 0 and ref["valid"][star_rows].all()
    assert min(faint_rows) >= 0 and not ref["valid"][faint_rows].any()
    assert 0 < ref["valid"].sum() < len(ref["valid"])
    assert cat.segment_flux_sum_valid == float(np.sum(cat.segment_flux[cat.valid]))
    assert cat.segment_flux_sum_valid < cat.segment_flux_sum
    # the same detections by the CPU restatement of source_info on the device's maps
    rlab, rn, _, _, _ = seg_ref.source_info(field, bkg.background, bkg.background_rms, n_pixels=1,
                                            kernel=sg.make_2dgaussian_kernel(1.2, 3))
    assert rn == cat.nlabels and np.array_equal(rlab, lab)
    # a device catalogue is read in place; the default window of 100
    dcat, dbkg = sg.source_info(field, 32, n_pixels=1, device_out=True, validate=True)
    assert dcat.f64_cols.is_cuda and dcat.validation.valid_dev.is_cuda
    r100 = validate_ref(field, pos, bkg.background, bkg.background_rms, 100)
    check(dcat.validation, r100)
    inplace = validate_sources(field, dcat, dbkg.background, dbkg.background_rms)
    check(inplace, r100)
    # a batch: every image as alone
    two = np.stack([field, field[::-1].copy()])
    bcat, _ = sg.source_info(two, 32, n_pixels=1, validate=True, validate_size=9)
    assert np.array_equal(bcat.valid[0], cat.valid) and len(bcat.valid[1]) == bcat.nlabels[1]
    assert bcat.segment_flux_sum_valid[0] == cat.segment_flux_sum_valid
