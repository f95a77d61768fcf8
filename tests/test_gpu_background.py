"""background.Background2D on the device against tests/golden/bkg2d_cases.npz
(made by tests/golden/make_golden_bkg.py from astropy.stats.SigmaClip,
scipy.ndimage.generic_filter / zoom and a numpy restatement of the fill).

Bars:
* survivor and iteration counts and the unfiltered background mesh: exact
  (the golden's membership margin is >= 4.4e-6, the std agrees to 1e-11);
* background_rms_mesh: rtol 1e-11 (two-pass sum of <= 4096 terms: n*eps =
  4.5e-13 per side);
* filled cells rtol 1e-11, cells the filter fed only unfilled values exact;
* maps against scipy's zoom on the 7x7 meshes: MAP_BAR * max|mesh|.  The
  kernels reproduce scipy's prefilter recursion (tests/bkg_ref.py does so to
  1e-13 on the CPU), so the bar is 10x the largest difference measured on the
  device (see MAP_BAR) rather than the 1e-7 a textbook boundary would need;
* maps of the 3x3 and 1x2 meshes against bkg_ref.zoom of the device's own
  filtered mesh at 1e-12 (the coefficient mesh is not an output of
  bsgp_background2d; bkg_ref.coefficients restates the prefilter).
"""
import numpy as np
import pytest

import bkg_ref

pytestmark = pytest.mark.gpu

# measured on MI355X, relative to max|mesh|: 1.26e-15 / 1.02e-15 (c1 bkg / rms),
# 1.12e-15 / 9.9e-16 (c2a), 1.12e-15 / 9.5e-16 (c2b); the bar is 10x the largest
MAP_BAR = 1.3e-14

CASES = {
    "c1": dict(box=(7, 8), kw={}),
    "c2a": dict(box=60, kw={}),
    "c2b": dict(box=60, kw=dict(exclude_percentile=100.0)),
    "c3": dict(box=7, kw=dict(exclude_percentile=20.0)),
    "c4": dict(box=64, kw={}),
}
RAWS = {"c1raw": "c1", "c2raw": "c2a", "c3raw": "c3", "c4raw": "c4"}


@pytest.fixture(scope="module")
def fx():
    return bkg_ref.cases()


def _inputs(fx, tag):
    from conftest import golden
    if tag.startswith("c2"):
        return golden("app_subdiv_inputs.npz")["img"], None
    if tag == "c3":
        d = fx["c3_data"].copy()
        d[fx["c3_nanmask"]] = np.nan
        return d, fx["c3_mask"]
    return fx[f"{tag}_data"], None


@pytest.fixture(scope="module")
def runs(fx):
    """Every case once: its own parameters, and the raw run (filter 1,
    exclude_percentile 100) that exposes the unfiltered box statistics."""
    from background import Background2D
    out = {}
    for tag, c in CASES.items():
        d, m = _inputs(fx, tag)
        out[tag] = Background2D(d, c["box"], filter_size=3, mask=m, **c["kw"])
    for raw, tag in RAWS.items():
        d, m = _inputs(fx, tag)
        out[raw] = Background2D(d, CASES[tag]["box"], filter_size=1, mask=m,
                                exclude_percentile=100.0)
    return out


@pytest.mark.parametrize("raw", sorted(RAWS))
def test_box_statistics(fx, runs, raw):
    """Counts exact, unfiltered median mesh bit for bit, std at rtol 1e-11."""
    b = runs[raw]
    kept = fx[f"{raw}_nsurv"] > 0
    assert kept.sum() >= kept.size - 1
    np.testing.assert_array_equal(b.mesh_excluded, ~kept)
    np.testing.assert_array_equal(b.mesh_npixels, fx[f"{raw}_nsurv"])
    np.testing.assert_array_equal(b.mesh_iterations, fx[f"{raw}_niter"])
    np.testing.assert_array_equal(b.background_mesh[kept], fx[f"{raw}_raw_med"][kept])
    pos = kept & (fx[f"{raw}_raw_std"] > 0)
    print(raw, "std rel", np.max(np.abs(b.background_rms_mesh[pos] / fx[f"{raw}_raw_std"][pos] - 1)))
    np.testing.assert_allclose(b.background_rms_mesh[kept], fx[f"{raw}_raw_std"][kept],
                               rtol=1e-11, atol=0)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_filled_and_filtered_meshes(fx, runs, tag):
    b = runs[tag]
    np.testing.assert_array_equal(b.mesh_excluded, fx[f"{tag}_excl"])
    np.testing.assert_array_equal(b.mesh_npixels, fx[f"{tag}_nsurv"])
    np.testing.assert_array_equal(b.mesh_iterations, fx[f"{tag}_niter"])
    pure = fx[f"{tag}_pure"]
    np.testing.assert_array_equal(b.background_mesh[pure], fx[f"{tag}_bkg_mesh"][pure])
    np.testing.assert_allclose(b.background_mesh, fx[f"{tag}_bkg_mesh"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(b.background_rms_mesh, fx[f"{tag}_rms_mesh"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(b.background_median, fx[f"{tag}_bkg_median"], rtol=1e-11)
    np.testing.assert_allclose(b.background_rms_median, fx[f"{tag}_rms_median"], rtol=1e-11)
    assert b.background_median == np.median(b.background_mesh)
    assert b.background_rms_median == np.median(b.background_rms_mesh)


def test_fill_of_the_masked_box(fx, runs):
    """Case 3's centre box is entirely masked: excluded, filled from its 8
    neighbours (4 at distance 1, 4 at sqrt 2), rtol 1e-11 on the filled cell;
    the raw run shows the filled value unfiltered."""
    raw = runs["c3raw"]
    assert raw.mesh_excluded[1, 1] and raw.mesh_excluded.sum() == 1
    m = raw.background_mesh
    w = np.array([[2 ** -0.5, 1, 2 ** -0.5], [1, 0, 1], [2 ** -0.5, 1, 2 ** -0.5]])
    np.testing.assert_allclose(m[1, 1], np.sum(w * np.where(w > 0, m, 0)) / w.sum(), rtol=1e-11)
    s = raw.background_rms_mesh
    np.testing.assert_allclose(s[1, 1], np.sum(w * np.where(w > 0, s, 0)) / w.sum(), rtol=1e-11)
    # constant box: all 49 pixels survive the inclusive bounds
    assert raw.mesh_npixels[0, 0] == 49 and m[0, 0] == 42.5 and s[0, 0] == 0.0
    assert raw.mesh_npixels[0, 2] <= 44


@pytest.mark.parametrize("tag", ["c1", "c2a", "c2b"])
def test_maps_match_scipy_zoom(fx, runs, tag):
    b = runs[tag]
    idx = fx["c2_idx"]
    for nm, got, mesh in (("bkg", b.background, b.background_mesh),
                          ("rms", b.background_rms, b.background_rms_mesh)):
        if tag.startswith("c2"):
            assert got.shape == (375, 375)
            got = got[np.ix_(idx, idx)]
        ref = fx[f"{tag}_{nm}"]
        scale = np.max(np.abs(fx[f"{tag}_{nm}_mesh"]))
        err = np.max(np.abs(got - ref)) / scale
        print(tag, nm, "map vs scipy, relative to max|mesh|:", err)
        # the filled cells of c2a carry their 1e-11 into the map
        bar = MAP_BAR if fx[f"{tag}_excl"].sum() == 0 else 1e-11
        assert err <= bar, (tag, nm, err)
        assert err <= 1e-7  # the bar a textbook prefilter boundary would have needed


@pytest.mark.parametrize("tag", sorted(CASES))
def test_maps_match_own_mesh_and_clamp(fx, runs, tag):
    """Every map against the numpy evaluation of the device's own filtered
    mesh at 1e-12 (for the 3x3 and 1x2 meshes the only map bar), inside the
    filtered mesh's range, and exactly constant along an axis of one cell."""
    b = runs[tag]
    box = CASES[tag]["box"]
    box = (box, box) if np.ndim(box) == 0 else box
    for got, mesh in ((b.background, b.background_mesh), (b.background_rms, b.background_rms_mesh)):
        ref = bkg_ref.zoom(mesh, box, got.shape)
        err = np.max(np.abs(got - ref)) / np.max(np.abs(mesh))
        print(tag, "map vs own mesh:", err)
        assert err <= 1e-12, (tag, err)
        assert got.min() >= mesh.min() and got.max() <= mesh.max()
        if mesh.shape[0] == 1:
            assert np.all(got == got[0])
    if tag.startswith("c2"):  # without the clamp the application tile's map leaves the range
        un = bkg_ref.zoom(b.background_mesh, box, b.background.shape, clip=False)
        assert un.min() < b.background_mesh.min() or un.max() > b.background_mesh.max()


def test_clip_false_leaves_the_range(fx, runs):
    from background import Background2D
    d, _ = _inputs(fx, "c2b")
    b = Background2D(d, 60, exclude_percentile=100.0, clip=False)
    lo, hi = fx["c2b_bkg_unclipped_range"]
    assert abs(b.background.min() - lo) <= 1e-11 * abs(lo) and abs(b.background.max() - hi) <= 1e-11 * hi
    np.testing.assert_array_equal(b.background_mesh, runs["c2b"].background_mesh)
    inside = (b.background >= b.background_mesh.min()) & (b.background <= b.background_mesh.max())
    np.testing.assert_array_equal(b.background[inside], runs["c2b"].background[inside])


def test_box_size_cap(fx):
    from background import Background2D
    import _bsgp
    d = np.zeros((65, 128), np.float32)
    d[:64] = fx["c4_data"]
    with pytest.raises(_bsgp.BsgpError, match="4096") as e:
        Background2D(d, (65, 64))
    assert e.value.code == _bsgp.BSGP_ERR_UNSUPPORTED


def _same(a, b):
    for k in ("background", "background_rms", "background_mesh", "background_rms_mesh",
              "mesh_npixels", "mesh_iterations", "mesh_excluded"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


def test_batch_equals_single_images_bitwise(fx):
    from background import Background2D
    d = fx["c5_data"]
    batch = Background2D(d, 7)
    assert batch.background.shape == (3, 21, 21) and batch.background_mesh.shape == (3, 3, 3)
    for i in range(3):
        one = Background2D(d[i], 7)
        for k in ("background", "background_rms", "background_mesh", "background_rms_mesh",
                  "mesh_npixels", "mesh_iterations", "mesh_excluded"):
            np.testing.assert_array_equal(getattr(batch, k)[i], getattr(one, k), err_msg=k)
        assert batch.background_median[i] == one.background_median
        assert batch.background_rms_median[i] == one.background_rms_median
        np.testing.assert_allclose(one.background_mesh, fx[f"c5i{i}_bkg_mesh"], rtol=1e-11)
        np.testing.assert_allclose(one.background_rms_mesh, fx[f"c5i{i}_rms_mesh"], rtol=1e-11)
        np.testing.assert_array_equal(one.mesh_npixels, fx[f"c5i{i}_nsurv"])


def test_float32_equals_float64_bitwise(fx):
    import _bsgp
    from background import Background2D
    d = fx["c5_data"]
    assert d.dtype == np.float32
    _same(Background2D(d, 7), Background2D(d.astype(np.float64), 7))
    # a CUDA tensor and device_out give the same bits as numpy in, numpy out
    t = Background2D(_bsgp.torch.from_numpy(d).cuda(), 7, device_out=True)
    assert t.background.is_cuda and t.background.dtype == _bsgp.torch.float64
    np.testing.assert_array_equal(t.background.cpu().numpy(), Background2D(d, 7).background)


def test_mask_equals_nan_bitwise(fx, runs):
    """Case 3's five NaN pixels masked instead (finite values under the mask)."""
    from background import Background2D
    mask = fx["c3_mask"] | fx["c3_nanmask"]
    b = Background2D(fx["c3_data"], 7, mask=mask, exclude_percentile=20.0)
    _same(b, runs["c3"])


def test_filter_1x1_leaves_the_box_medians(fx, runs):
    from background import Background2D
    d, m = _inputs(fx, "c3")
    b = Background2D(d, 7, filter_size=(1, 1), mask=m, exclude_percentile=20.0)
    kept = ~fx["c3_excl"]
    np.testing.assert_array_equal(b.background_mesh[kept], fx["c3_raw_med"][kept])
    np.testing.assert_allclose(b.background_mesh, fx["c3_bkg_filled"], rtol=1e-11)
    assert not np.array_equal(b.background_mesh, runs["c3"].background_mesh)


def test_every_box_excluded_raises(fx):
    from background import Background2D
    d = np.stack([fx["c5_data"][0], np.full((21, 21), np.nan, np.float32)])
    with pytest.raises(ValueError, match="image 1"):
        Background2D(d, 7)
    with pytest.raises(ValueError, match="image 0"):
        Background2D(fx["c5_data"][0], 7, mask=np.ones((21, 21), bool))


def test_subdivisions_estimate_equals_explicit_map():
    """sgp_subdivisions(bkg="estimate") on a 2x2-tile field is the call given
    Background2D(field, ...).background, bit for bit."""
    import subdivisions
    from background import Background2D
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[:96, :96]
    g = np.exp(-((np.arange(9) - 4.0) ** 2) / 4.0)
    psf = np.outer(g, g) / np.sum(np.outer(g, g))
    field = rng.poisson(100.0 + 0.2 * yy + 0.1 * xx).astype(np.float64)
    field[30, 40] += 3000.0
    field[70, 20] += 2000.0
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, MAXIT=3, alpha=10.0,
              ccd_sat_level=65000.0, use_original_SGP_Afunction=False, schedule_lr=True,
              adapt_beta=False, betaParam=1.05, verbose=False)
    assert len(subdivisions.subdivision_boxes((96, 96), (64, 64), 32)) == 4
    m1, f1, o1 = subdivisions.sgp_subdivisions(field, psf, "estimate", (64, 64), 32,
                                               bkg_box_size=16, bkg_filter_size=3, **kw)
    bmap = Background2D(field, 16, filter_size=3).background
    assert bmap.dtype == np.float64 and bmap.shape == (96, 96)
    m2, f2, o2 = subdivisions.sgp_subdivisions(field, psf, bmap, (64, 64), 32, **kw)
    np.testing.assert_array_equal(m1, m2)
    np.testing.assert_array_equal(f1, f2)
    np.testing.assert_array_equal(o1["discr"], o2["discr"])
    assert np.all(np.isfinite(m1)) and not np.array_equal(
        m1, subdivisions.sgp_subdivisions(field, psf, 100.0, (64, 64), 32, **kw)[0])
