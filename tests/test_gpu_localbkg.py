"""The local background of the source catalogue on the device
(``SourceCatalog(..., localbkg_width=L)``, bsgp_segment_local_background,
DESIGN §3.8 L1 to L6) against the restatement tests/localbkg_ref.py: the
synthetic cases of tests/golden/localbkg_cases.npz, the cap, and the published
frame end to end against the catalogue photutils wrote for it
(tests/golden/SUBDIV_ORIGCAT.csv).

Device and restatement select the same pixels, so both counts are equal
exactly; the mean differs by summation order, and the bars of ``lb`` and of
the corrected columns are derived in localbkg_ref from that, not chosen."""
import os
import warnings

import numpy as np
import pytest

import localbkg_ref as ref
import seg_ref
from conftest import GOLDEN, golden, ref_kwargs

pytestmark = pytest.mark.gpu

TAGS = ("widths", "widths_half", "borders", "crossed", "few", "bright", "cascade", "constant",
        "skewed", "nonfinite", "one")
FLOAT_COLS = ("segment_flux", "min_value", "max_value")


@pytest.fixture(scope="module")
def sg():
    import _bsgp
    import segmentation
    _bsgp.require_gpu()
    return segmentation


@pytest.fixture(scope="module")
def fx():
    return golden("localbkg_cases.npz")


def restate(data, labels, width):
    """(catalogue, result of ref.local_background, corrected columns, their bars)."""
    cat = seg_ref.catalog(data, labels)
    box = np.stack([cat["bbox_xmin"], cat["bbox_xmax"], cat["bbox_ymin"], cat["bbox_ymax"]], 1)
    res = ref.local_background(data, labels, box, cat["area"], width)
    cor = ref.corrected(cat, res["lb"])
    bars = ref.column_bars(cat, res["lb"], res["bar"], seg_ref.column_bars(cat, data.shape)["flux"])
    return cat, res, cor, bars


def check_catalogue(sg, cat, cat0, data, labels, width):
    """A device catalogue with a width against the restatement and against the
    device catalogue without one."""
    rc, res, cor, bars = restate(np.asarray(data, dtype=np.float64), labels, width)
    lb, npix = cat.local_background, cat.localbkg_npix
    print("lb", lb, "restated", res["lb"], "bar", res["bar"], "npix", npix.tolist())
    assert np.array_equal(npix[:, 0], res["ngather"]) and np.array_equal(npix[:, 1], res["nsurv"])
    assert cat.localbkg_status == res["status"]
    assert np.all(np.abs(lb - res["lb"]) <= res["bar"]), np.abs(lb - res["lb"]) / res["bar"]
    for nm in FLOAT_COLS:
        assert np.all(np.abs(cat[nm] - cor[nm]) <= bars[nm]), nm
    # L6 is these operations on the device's own numbers, to the bit
    area = cat0.area.astype(np.float64)
    assert np.array_equal(cat.segment_flux, cat0.segment_flux - area * lb)
    assert np.array_equal(cat.min_value, cat0.min_value - lb)
    assert np.array_equal(cat.max_value, cat0.max_value - lb)
    for nm in sg.COLUMNS:  # exactly the three columns are rewritten
        if nm not in FLOAT_COLS:
            assert np.array_equal(cat[nm], cat0[nm], equal_nan=True), nm
    assert cat.segment_flux_sum == float(np.sum(cat.segment_flux))
    return res


@pytest.mark.parametrize("tag", TAGS)
def test_synthetic_cases(sg, fx, tag):
    d, lab, w = fx[f"{tag}_data"], fx[f"{tag}_labels"].astype(np.int32), float(fx[f"{tag}_width"])
    cat, cat0 = sg.SourceCatalog(d, lab, localbkg_width=w), sg.SourceCatalog(d, lab)
    res = check_catalogue(sg, cat, cat0, d, lab, w)
    for k in ("ngather", "nsurv"):
        assert np.array_equal(res[k], fx[f"{tag}_{k}"])
    assert np.all(np.abs(cat.local_background - fx[f"{tag}_lb"]) <= res["bar"])
    with pytest.raises(KeyError, match="localbkg_width"):
        cat0["local_background"]
    if tag == "few":
        assert cat.localbkg_status == sg._B.BSGP_LOCALBKG_FEW and np.all(cat.local_background == 0.0)
        assert np.array_equal(cat.segment_flux, cat0.segment_flux)
    if tag == "constant":  # std == 0: the mean of equal values, exactly
        assert cat.local_background[0] == 3.0 and cat.min_value[0] == 77.0


def raw_call(sg, data_t, lab_t, width, apply=1, maxiters=10, min_pixels=10):
    """bsgp_segment_catalog on the float64 widening, then the local background
    of data_t in its own dtype: (lb, npix, status, f64 columns) on the host."""
    torch, B_ = sg._B.torch, sg._B
    Bn, H, W = data_t.shape
    cap = max(1, int(lab_t.max()))
    d64 = data_t.to(torch.float64)
    ic = torch.empty((Bn, cap, 5), dtype=torch.int32, device="cuda")
    fc = torch.empty((Bn, cap, 8), dtype=torch.float64, device="cuda")
    st = torch.empty((Bn,), dtype=torch.int32, device="cuda")
    B_.check(B_.lib().bsgp_segment_catalog(B_._ptr(d64), None, B_._ptr(lab_t), Bn, H, W, cap, None,
                                           B_._ptr(ic), B_._ptr(fc), B_._ptr(st),
                                           B_.current_stream()))
    lb = torch.full((Bn, cap), -7.0, dtype=torch.float64, device="cuda")
    npx = torch.full((Bn, cap, 2), -7, dtype=torch.int32, device="cuda")
    lst = torch.full((Bn,), -7, dtype=torch.int32, device="cuda")
    B_.check(B_.lib().bsgp_segment_local_background(
        B_._ptr(data_t), sg._dtype(data_t), B_._ptr(lab_t), Bn, H, W, cap, None, B_._ptr(ic),
        B_._ptr(fc) if apply else None, float(width), 3.0, maxiters, min_pixels, apply, B_._ptr(lb),
        B_._ptr(npx), B_._ptr(lst), B_.current_stream()))
    return lb.cpu().numpy(), npx.cpu().numpy(), lst.cpu().numpy(), fc.cpu().numpy()


def test_float32_gives_the_bits_of_its_widening(sg, fx):
    torch = sg._B.torch
    d = torch.from_numpy(fx["f32_data"]).to("cuda")[None]
    lab = torch.from_numpy(fx["f32_labels"].astype(np.int32)).to("cuda")[None]
    assert d.dtype == torch.float32
    a = raw_call(sg, d, lab, 2.0)
    b = raw_call(sg, d.to(torch.float64), lab, 2.0)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert np.array_equal(a[1][0, :, 0], fx["f32_ngather"]) and np.array_equal(a[1][0, :, 1],
                                                                                fx["f32_nsurv"])
    rc, res, cor, bars = restate(fx["f32_data"].astype(np.float64), fx["f32_labels"].astype(np.int32), 2.0)
    assert np.all(np.abs(a[0][0] - res["lb"]) <= res["bar"])
    # apply == 0 measures and leaves the columns alone (f64_cols may be NULL)
    c = raw_call(sg, d, lab, 2.0, apply=0)
    assert np.array_equal(c[0], a[0]) and np.array_equal(c[1], a[1])
    area = rc["area"].astype(np.float64)[None]
    assert np.array_equal(a[3][..., 0], c[3][..., 0] - area * a[0])  # L6, to the bit
    assert np.array_equal(a[3][..., 1], c[3][..., 1] - a[0])
    assert np.array_equal(c[3][..., 3:], a[3][..., 3:])
    # maxiters = 0: no clipping; min_pixels above a count: FEW and 0.0
    e = raw_call(sg, d, lab, 2.0, maxiters=0)
    assert np.array_equal(e[1][0, :, 0], e[1][0, :, 1])
    f = raw_call(sg, d, lab, 2.0, min_pixels=41)
    assert f[2][0] == sg._B.BSGP_LOCALBKG_FEW
    assert np.array_equal(f[0][0] == 0.0, fx["f32_ngather"] < 41) and (f[0][0] == 0.0).sum() == 2


def test_batch_gives_each_image_the_bits_it_gets_alone(sg, fx):
    torch = sg._B.torch
    data = np.stack([fx["widths_data"], fx["one_data"], fx["one_data"]])
    labels = np.stack([fx["widths_labels"], np.zeros_like(fx["one_labels"]), fx["one_labels"]])
    labels = labels.astype(np.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("error", sg.LocalBackgroundCapWarning)
        bat = sg.SourceCatalog(data, labels, localbkg_width=2.0, device_out=True)
    assert bat.nlabels.tolist() == [4, 0, 1] and bat.localbkg_status.tolist() == [0, 0, 0]
    assert torch.is_tensor(bat.local_background_dev) and bat.local_background_dev.is_cuda
    assert tuple(bat.local_background_dev.shape) == (3, 4)
    assert tuple(bat.int_cols.shape) == (3, 4, 5) and tuple(bat.f64_cols.shape) == (3, 4, 8)
    assert bat.f64_cols.is_cuda and bat.int_cols.is_cuda
    dev = bat.local_background_dev.cpu().numpy()
    assert np.all(dev[1] == 0.0) and np.all(dev[2, 1:] == 0.0)
    for b in (0, 2):
        one = sg.SourceCatalog(data[b], labels[b], localbkg_width=2.0)
        assert np.array_equal(dev[b, :len(one)], one.local_background)
        for nm in sg.COLUMNS + ("local_background",):
            assert np.array_equal(bat[nm][b], one[nm], equal_nan=True), (b, nm)
        assert np.array_equal(bat.localbkg_npix[b], one.localbkg_npix)
        assert bat.segment_flux_sum[b] == one.segment_flux_sum
    assert len(bat.local_background[1]) == 0 and bat.segment_flux_sum[1] == 0.0
    assert np.array_equal(bat.f64_cols.cpu().numpy()[0, :, 0], bat.segment_flux[0])
    # a lone image without a label
    none = sg.SourceCatalog(data[1], labels[1], localbkg_width=2.0)
    assert len(none.local_background) == 0 and none.localbkg_status == 0


def cap_image():
    rng = np.random.default_rng(5)
    d = 20.0 + rng.standard_normal((128, 128))
    lab = np.zeros((128, 128), np.int32)
    lab[54:74, 54:74] = 1
    d[lab == 1] += 100.0
    return d, lab


def test_annulus_over_the_cap_is_flagged_and_left_uncorrected(sg):
    d, lab = cap_image()
    assert ref.annulus(d.shape, (54, 73, 54, 73), 40.0).sum() == 11200 > sg.LOCALBKG_MAX
    with pytest.warns(sg.LocalBackgroundCapWarning, match="1 source"):
        cat = sg.SourceCatalog(d, lab, localbkg_width=40)
    cat0 = sg.SourceCatalog(d, lab)
    assert cat.localbkg_status == sg._B.BSGP_LOCALBKG_OVER_CAP
    assert cat.local_background.tolist() == [0.0] and cat.localbkg_npix.tolist() == [[11200, 0]]
    for nm in sg.COLUMNS:
        assert np.array_equal(cat[nm], cat0[nm], equal_nan=True), nm


def test_annulus_of_exactly_the_cap_is_served(sg):
    d, lab = cap_image()
    ann = ref.annulus(d.shape, (54, 73, 54, 73), 40.0)
    outer = np.zeros_like(ann)
    outer[9:119, 9:119] = True
    inner = np.zeros_like(ann)
    inner[49:79, 49:79] = True
    assert np.array_equal(ann, outer & ~inner)
    # a second segment takes everything outside the outer rectangle and the
    # first 3008 annulus pixels in raster order: 8192 remain.  Its own box is the
    # image, so its annulus is empty (FEW).
    surplus = np.flatnonzero(ann.ravel())[:11200 - sg.LOCALBKG_MAX]
    lab.ravel()[surplus] = 2
    lab[~outer] = 2
    with warnings.catch_warnings():
        warnings.simplefilter("error", sg.LocalBackgroundCapWarning)
        cat = sg.SourceCatalog(d, lab, localbkg_width=40)
    cat0 = sg.SourceCatalog(d, lab)
    assert cat.localbkg_npix[0, 0] == sg.LOCALBKG_MAX == 8192
    assert cat.localbkg_status == sg._B.BSGP_LOCALBKG_FEW and cat.localbkg_npix[1].tolist() == [0, 0]
    check_catalogue(sg, cat, cat0, d, lab, 40.0)
    assert 19.5 < cat.local_background[0] < 20.5


# ------------------------------------------------------- the published frame
@pytest.fixture(scope="module")
def frame(sg):
    import fits_io
    _, img = fits_io.read_fits(os.path.join(GOLDEN, "SUBDIV_ORIGIMG.fits"))
    with warnings.catch_warnings():
        warnings.simplefilter("error", sg.LocalBackgroundCapWarning)
        cat, bkg = sg.source_info(img, 60, 5, deblend=True, localbkg_width=5)
    return img, cat


def test_published_frame_labels_equal_the_fixture(fx, frame):
    img, cat = frame
    assert cat.nlabels == 104
    assert np.array_equal(cat.segment_img.data, fx["pub_labels"].astype(np.int32))


def test_published_frame_against_the_restatement(sg, frame):
    """The restatement on the device's own background-subtracted image and
    labels: the same pixels and values, so the derived bars apply."""
    img, cat = frame
    labels = np.asarray(cat.segment_img.data)
    rc, res, cor, bars = restate(cat.data, labels, 5.0)
    assert cat.localbkg_status == 0 == res["status"]
    assert np.array_equal(cat.localbkg_npix[:, 0], res["ngather"])
    assert np.array_equal(cat.localbkg_npix[:, 1], res["nsurv"])
    err = np.abs(cat.local_background - res["lb"])
    print("largest lb error / bar:", (err / res["bar"]).max())
    assert np.all(err <= res["bar"])
    for nm in FLOAT_COLS:
        assert np.all(np.abs(cat[nm] - cor[nm]) <= bars[nm]), nm
    # the other columns are those of the catalogue without a width
    cat0 = sg.SourceCatalog(cat.data, cat.segment_img, convolved_data=cat.convolved_data)
    for nm in sg.COLUMNS:
        if nm not in FLOAT_COLS:
            assert np.array_equal(cat[nm], cat0[nm], equal_nan=True), nm
    assert np.array_equal(cat.segment_flux,
                          cat0.segment_flux - cat0.area.astype(np.float64) * cat.local_background)


def test_published_frame_against_the_published_catalogue(frame):
    img, cat = frame
    pub = ref.read_published(os.path.join(GOLDEN, "SUBDIV_ORIGCAT.csv"))
    cols = {k: np.asarray(cat[k]) for k in ("area", "bbox_xmin", "bbox_xmax", "bbox_ymin", "bbox_ymax")}
    got = ref.check_against_published(cols, cat.local_background, cat.segment_flux,
                                      cat.min_value + cat.local_background, pub)
    assert got["matched"] == 97
    assert abs(cat.segment_flux_sum - pub["segment_flux"].sum()) / pub["segment_flux"].sum() <= 5e-4


def test_flux_sums_and_the_subdivisions_constraint(sg, frame, monkeypatch, tmp_path):
    import sgp
    import subdivisions
    from test_gpu_segmentation import field96
    img, cat = frame
    sums = sg.segment_flux_sums(img[None], 60, 5, localbkg_width=5, deblend=True)
    assert sums.shape == (1,) and sums[0] == cat.segment_flux_sum
    plain = sg.segment_flux_sums(img[None], 60, 5)
    assert plain[0] > sums[0] * 1.02  # the uncorrected sum is 2.8 % higher

    monkeypatch.chdir(tmp_path)
    fx64 = golden("ref_lin64_beta.npz")
    kw = ref_kwargs(fx64)
    kw.update(MAXIT=3, verbose=False)
    beta = kw.pop("betaParam")
    field = field96()[:64]
    seen = {}
    real = sgp.sgp_betaDiv_batch

    def spy(gns, *a, **k):
        seen["flux"], seen["gns"] = np.asarray(k["flux"]), gns
        return real(gns, *a, **k)

    monkeypatch.setattr(sgp, "sgp_betaDiv_batch", spy)
    subdivisions.sgp_subdivisions(field, fx64["psf"], "estimate", subdiv_shape=(64, 64), overlap=32,
                                  betaParams=beta, bkg_box_size=16, flux="segments",
                                  flux_localbkg_width=5, flux_deblend=True, **kw)
    assert seen["flux"].shape == (2,)
    want = sg.segment_flux_sums(seen["gns"], 16, 5, localbkg_width=5, deblend=True)
    assert np.array_equal(seen["flux"], want)
    assert not np.array_equal(want, sg.segment_flux_sums(seen["gns"], 16, 5))
    score = sg.catalog_flux_fraction_score(None, 16, localbkg_width=5, deblend=True)
    s = score.batch(seen["gns"], seen["gns"])
    num = sg.segment_flux_sums(seen["gns"], 16, 1, localbkg_width=5, deblend=True)
    assert s.shape == (2,) and np.array_equal(s, 1.0 - num / want)
