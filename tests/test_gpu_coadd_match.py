"""The background-matched co-add on the device against
its numpy restatement (tests/coadd_ref.py): offsets bit-equal to numpy.median,
corrections within reproject's own convergence threshold of the least-squares
solution, the mosaic bit-equal to the restated co-add fed the device's
corrections, and no seams where the tiles differ by constants only."""
import warnings

import numpy as np
import pytest

import coadd_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def S():
    import _bsgp
    import subdivisions
    _bsgp.require_gpu()
    return subdivisions


def _grid(shape, tile, overlap):
    import subdivisions
    return subdivisions.subdivision_boxes(shape, tile, overlap), tile, shape


def _field(shape):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    return 50 + 0.1 * xx + 0.05 * yy + 3 * np.sin(xx / 9.0) * np.cos(yy / 7.0)


def _cut(field, boxes, tile):
    t = np.zeros((len(boxes),) + tuple(tile))
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        t[k, :y1 - y0, :x1 - x0] = field[y0:y1, x0:x1]
    return t


# name -> (boxes, tile shape, field shape)
HAND = np.asarray([[0, 0, 10, 10], [6, 0, 16, 10], [6, 7, 16, 17],   # three that all overlap
                   [40, 40, 50, 50], [49, 49, 59, 59],               # a 1-pixel overlap
                   [100, 0, 110, 10]], dtype=np.int32)               # a tile alone
LAYOUTS = {
    "grid12": lambda: _grid((100, 130), (45, 39), 7),   # 29 pairs of 49..1092 values, 14 odd
    "grid4": lambda: _grid((64, 64), (48, 48), 8),      # four inward-shifted tiles
    "grid25": lambda: _grid((120, 120), (32, 32), 6),   # shifted last row and column
    "hand": lambda: (HAND, (10, 10), (60, 110)),
    "big": lambda: (np.asarray([[0, 0, 300, 300], [1, 0, 301, 300]], np.int32), (300, 300),
                    (300, 301)),                       # 89 700 values in one overlap
}
_CASES = {}


def case(name, data):
    """Tiles of a layout: 'noisy' = a smooth field + a constant per tile +
    noise (the middle values differ), 'ties' = the same rounded to integers
    (the two middle values are often equal), 'clean' = field + constant.
    With the restated B1-B3 computed once."""
    key = (name, data)
    if key not in _CASES:
        boxes, tile, shape = LAYOUTS[name]()
        rng = np.random.default_rng(sum(map(ord, name)))
        field = _field(shape)
        consts = rng.normal(0, 5, len(boxes))
        t = _cut(field, boxes, tile) + consts[:, None, None]
        if data != "clean":
            t = t + rng.normal(0, 0.3, t.shape)
        if data == "ties":
            t = np.rint(t)
        pr, rects = coadd_ref.pairs(boxes)
        off, st = coadd_ref.offsets(t, boxes, pr, rects)
        c, st2 = coadd_ref.corrections(len(boxes), pr, off)
        comp, ncomp = coadd_ref.components(len(boxes), pr)
        for a in (t, off, c, field):
            a.setflags(write=False)
        _CASES[key] = dict(boxes=boxes, tile=tile, shape=shape, tiles=t, field=field, pairs=pr,
                           rects=rects, offsets=off, c=c, status=st | st2, comp=comp, ncomp=ncomp)
    return _CASES[key]


def _match(S, cs, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", S.TileMatchWarning)
        return S.match_tile_backgrounds(cs["tiles"], cs["boxes"], **kw)


ALL = [(n, d) for n in LAYOUTS for d in ("noisy", "ties")]


@pytest.mark.parametrize("name,data", ALL)
def test_offsets_bit_equal_to_numpy_median(S, name, data):
    cs = case(name, data)
    m = _match(S, cs)
    np.testing.assert_array_equal(m.pairs, cs["pairs"])
    assert m.offsets.dtype == np.float64 and m.offsets.shape == (len(cs["pairs"]),)
    np.testing.assert_array_equal(m.offsets, cs["offsets"])
    om = m.offset_matrix
    n = len(cs["boxes"])
    assert om.shape == (n, n) and np.isnan(om).sum() == n * n - 2 * len(cs["pairs"])
    for (i, j), o in zip(cs["pairs"], cs["offsets"]):
        assert om[i, j] == o and om[j, i] == -o
    if data == "ties" and name in ("grid12", "big"):  # both middle values are one value
        cnt = (cs["rects"][:, 2] - cs["rects"][:, 0]) * (cs["rects"][:, 3] - cs["rects"][:, 1])
        even = cnt % 2 == 0
        assert np.any(cs["offsets"][even] == np.rint(cs["offsets"][even]))


@pytest.mark.parametrize("name,data", ALL)
def test_corrections_match_least_squares(S, name, data):
    """Within 1e-10 * max|c| (the threshold at which reproject's own solver
    stops) of lstsq on the Laplacian; zero mean in every component.  The mean
    is taken off in float64: what is left of a component's mean is bounded by
    the rounding of its n subtractions and of the mean itself, n * eps * max|c|."""
    cs = case(name, data)
    m = _match(S, cs)
    scale = np.abs(cs["c"]).max()
    err = np.abs(m.corrections - cs["c"]).max()
    print(f"{name}/{data}: |c - lstsq| / max|c| = {err / scale:.2e}, CG iterations "
          f"{int(m.solve_info[0])}, relative residual {m.solve_info[1]:.2e}")
    assert err <= 1e-10 * scale
    np.testing.assert_array_equal(m.status, cs["status"])
    assert not np.any(m.status & 4) and int(m.solve_info[0]) <= len(cs["boxes"])
    n = len(cs["boxes"])
    for k in range(cs["ncomp"]):
        assert abs(m.corrections[cs["comp"] == k].mean()) <= n * EPS * scale


def test_isolated_tile_is_zero_flagged_and_warned(S):
    import _bsgp
    cs = case("hand", "noisy")
    with pytest.warns(S.TileMatchWarning, match="overlap no other"):
        m = S.match_tile_backgrounds(cs["tiles"], cs["boxes"])
    assert m.corrections[5] == 0.0 and m.status[5] == _bsgp.BSGP_COADD_ISOLATED
    assert not m.status[:5].any()
    # overlap 0: no pair at all, every tile alone
    boxes = S.subdivision_boxes((60, 90), (30, 30), 0)
    t = _cut(_field((60, 90)), boxes, (30, 30))
    with pytest.warns(S.TileMatchWarning):
        m = S.match_tile_backgrounds(t, boxes)
    assert m.offsets.shape == (0,) and not m.corrections.any()
    assert np.all(m.status == _bsgp.BSGP_COADD_ISOLATED)
    mean, foot = S.coadd_tiles(t, boxes, (60, 90), match_background=True)
    np.testing.assert_array_equal(mean.cpu().numpy(), _field((60, 90)))


@pytest.mark.parametrize("name", ["grid12", "hand"])
def test_background_reference(S, name):
    cs = case(name, "noisy")
    free = _match(S, cs)
    for k in (0, 2):
        m = _match(S, cs, background_reference=k)
        assert m.corrections[k] == 0.0
        np.testing.assert_array_equal(m.corrections, free.corrections - free.corrections[k])
        np.testing.assert_array_equal(m.offsets, free.offsets)
    with pytest.raises(ValueError, match="background_reference"):
        S.match_tile_backgrounds(cs["tiles"], cs["boxes"], background_reference=len(cs["boxes"]))


@pytest.mark.parametrize("name,data", [("grid12", "noisy"), ("grid12", "ties"), ("grid4", "noisy"),
                                       ("grid25", "noisy"), ("hand", "noisy"), ("big", "ties")])
def test_mosaic_bit_equal_to_restated_coadd(S, name, data):
    cs = case(name, data)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", S.TileMatchWarning)
        mean, foot = S.coadd_tiles(cs["tiles"], cs["boxes"], cs["shape"], match_background=True)
        m = mean._match.to_host()
    np.testing.assert_array_equal(m.offsets, cs["offsets"])
    ref_mean, ref_foot = coadd_ref.coadd(cs["tiles"], cs["boxes"], cs["shape"], m.corrections)
    np.testing.assert_array_equal(mean.cpu().numpy(), ref_mean)
    np.testing.assert_array_equal(foot.cpu().numpy(), ref_foot)


def test_mosaic_with_more_tiles_than_the_lds_holds_corrections_for(S):
    """B4 alone through the C ABI: 12 tiles (corrections staged in LDS) and
    6900 two-pixel tiles (past the staging limit: read from global memory)."""
    import _bsgp as B
    torch = B.torch
    rng = np.random.default_rng(5)
    for n in (12, 6900):
        boxes = np.stack([np.arange(n), np.zeros(n, int), np.arange(n) + 2, np.ones(n, int)],
                         axis=1).astype(np.int32)
        t = rng.normal(10, 1, (n, 1, 2))
        c = rng.normal(0, 1, n)
        td, cd, bd = B.to_dev(t), B.to_dev(c), torch.from_numpy(boxes).to("cuda")
        mean = torch.empty((1, n + 1), dtype=torch.float64, device="cuda")
        foot = torch.empty_like(mean)
        B.check(B.lib().bsgp_coadd_tiles_matched(B._ptr(td), n, 1, 2, B._ptr(bd), B._ptr(cd), 1,
                                                 n + 1, B._ptr(mean), B._ptr(foot),
                                                 B.current_stream()))
        ref_mean, ref_foot = coadd_ref.coadd(t, boxes, (1, n + 1), c)
        np.testing.assert_array_equal(mean.cpu().numpy(), ref_mean)
        np.testing.assert_array_equal(foot.cpu().numpy(), ref_foot)


@pytest.mark.parametrize("name", ["grid12", "grid4", "grid25"])
def test_no_seams_where_tiles_differ_by_constants(S, name):
    """Noise-free tiles (field + a constant each): the matched mosaic is the
    field up to ONE additive constant, to 1e-12 of the field's size; the plain
    mean keeps steps of the size of the constants."""
    cs = case(name, "clean")
    mean, foot = S.coadd_tiles(cs["tiles"], cs["boxes"], cs["shape"], match_background=True)
    plain, _ = S.coadd_tiles(cs["tiles"], cs["boxes"], cs["shape"])
    assert np.all(foot.cpu().numpy() > 0)
    scale = np.abs(cs["field"]).max()
    d = mean.cpu().numpy() - cs["field"]
    dp = plain.cpu().numpy() - cs["field"]
    print(f"{name}: matched spread {np.ptp(d) / scale:.2e}, plain spread {np.ptp(dp) / scale:.2e}")
    assert np.ptp(d) <= 1e-12 * scale
    assert np.ptp(dp) > 1e-3 * scale


def test_nan_in_one_overlap_drops_that_pair_only(S):
    import _bsgp
    cs = case("grid12", "noisy")
    t = cs["tiles"].copy()
    # tile 0 is [0, 39) x [0, 45); (y 5, x 35) lies in its overlap with tile 1 and no other
    p01 = [tuple(p) for p in cs["pairs"]].index((0, 1))
    x0, y0, x1, y1 = cs["rects"][p01]
    assert x0 <= 35 < x1 and y0 <= 5 < y1
    assert sum(r[0] <= 35 < r[2] and r[1] <= 5 < r[3] and 0 in cs["pairs"][k]
               for k, r in enumerate(cs["rects"])) == 1
    t[0, 5, 35] = np.nan
    with pytest.warns(S.TileMatchWarning, match="1 pair"):
        m = S.match_tile_backgrounds(t, cs["boxes"])
    assert np.isnan(m.offsets[p01])
    keep = np.arange(len(cs["pairs"])) != p01
    np.testing.assert_array_equal(m.offsets[keep], cs["offsets"][keep])
    want = np.zeros(len(cs["boxes"]), np.int32)
    want[[0, 1]] = _bsgp.BSGP_COADD_NONFINITE
    np.testing.assert_array_equal(m.status, want)
    c, _ = coadd_ref.corrections(len(cs["boxes"]), cs["pairs"], m.offsets)
    assert np.abs(m.corrections - c).max() <= 1e-10 * np.abs(c).max()
    assert np.all(np.isfinite(m.corrections))


def test_default_is_todays_coadd(S):
    import tiles_oracle
    cs = case("grid12", "noisy")
    a, fa = S.coadd_tiles(cs["tiles"], cs["boxes"], cs["shape"])
    b, fb = S.coadd_tiles(cs["tiles"], cs["boxes"], cs["shape"], match_background=False)
    m_ref, c_ref = tiles_oracle.coadd_mean(cs["tiles"], cs["boxes"], cs["shape"])
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == m_ref.tobytes()
    assert fa.cpu().numpy().tobytes() == fb.cpu().numpy().tobytes()
    np.testing.assert_array_equal(fa.cpu().numpy(), c_ref)
    assert not hasattr(b, "_match")


def test_sgp_subdivisions_matched(S):
    """The whole chain with match_background=True on the 100 x 130 field:
    finite output, and out["bkg_match"] reproduces the mosaic."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[:100, :130]
    g = np.exp(-((np.arange(9) - 4.0) ** 2) / 4.0)
    psf = np.outer(g, g) / np.sum(np.outer(g, g))
    field = rng.poisson(100.0 + 0.2 * yy + 0.1 * xx).astype(np.float64)
    field[30, 40] += 3000.0
    field[70, 100] += 2000.0
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, MAXIT=5, alpha=10.0,
              ccd_sat_level=65000.0, use_original_SGP_Afunction=False, schedule_lr=True,
              adapt_beta=False, betaParam=1.05, verbose=False)
    mosaic, foot, out = S.sgp_subdivisions(field, psf, 100.0, (45, 39), 7, match_background=True,
                                           **kw)
    boxes = S.subdivision_boxes((100, 130), (45, 39), 7)
    m = out["bkg_match"]
    assert np.all(np.isfinite(mosaic)) and np.all(foot > 0)
    assert m["corrections"].shape == (12,) and np.all(np.isfinite(m["corrections"]))
    assert not m.status.any() and len(m.pairs) == 29
    off, _ = coadd_ref.offsets(out["x"], boxes)
    np.testing.assert_array_equal(m["offsets"], off)
    ref_mean, ref_foot = coadd_ref.coadd(out["x"], boxes, (100, 130), m["corrections"])
    np.testing.assert_array_equal(mosaic, ref_mean)
    np.testing.assert_array_equal(foot, ref_foot)
    plain = S.sgp_subdivisions(field, psf, 100.0, (45, 39), 7, **kw)
    assert "bkg_match" not in plain[2] and not np.array_equal(plain[0], mosaic)
    # the multi-start chain: the match is that of the chosen candidates
    kw.pop("betaParam")
    mos, ft, info = S.sgp_subdivisions_multistart(field, psf, 100.0, betas=[1.05, 1.2],
                                                  subdiv_shape=(45, 39), overlap=7,
                                                  match_background=True, background_reference=3,
                                                  **kw)
    mm = info["bkg_match"]
    assert mm.corrections[3] == 0.0 and not mm.status.any()
    ref_mean, _ = coadd_ref.coadd(info["x"], boxes, (100, 130), mm.corrections)
    np.testing.assert_array_equal(mos, ref_mean)
    np.testing.assert_array_equal(mm.offsets, coadd_ref.offsets(info["x"], boxes)[0])


def test_device_out_keeps_the_match_on_the_device(S):
    import _bsgp
    cs = case("grid12", "noisy")
    m = S.match_tile_backgrounds(_bsgp.to_dev(cs["tiles"]), cs["boxes"], device_out=True)
    torch = _bsgp.torch
    assert all(torch.is_tensor(v) and v.is_cuda
               for v in (m.offsets, m.corrections, m.status, m.solve_info, m.offset_matrix))
    h = m.to_host()
    np.testing.assert_array_equal(h.offsets, cs["offsets"])
    np.testing.assert_array_equal(m.offset_matrix.cpu().numpy(), h.offset_matrix)
    again = S.match_tile_backgrounds(cs["tiles"], cs["boxes"])  # (the layout is cached now)
    np.testing.assert_array_equal(again.corrections, h.corrections)
