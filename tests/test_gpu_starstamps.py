"""The star-stamp application's loop on the MI355X (DESIGN §3.11;
application_sgp_star_stamps.py:56-148): the cutouts and the choice among the
candidates against their numpy restatements (tests/starstamps_ref.py), bit for
bit, and the driver against the same chain written out from the public calls it
batches."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

import starstamps_ref as ref

pytestmark = pytest.mark.gpu

MAXIT = 30


@pytest.fixture(scope="module")
def mods():
    import _bsgp
    _bsgp.require_gpu()
    import segmentation
    import sgp
    import stamps
    return _bsgp, sgp, segmentation, stamps


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------- cutouts
# (x, y) on a 48 x 64 image (H = 48, W = 64).  With size 31 a box starts at
# ceil(pos - 15.5): it is full for 15 <= x <= 48.5 and 15 <= y <= 32.5.
CUT_POSITIONS = [
    (32, 24), (20, 16), (47, 31),                       # integers
    (20.49, 24), (20.5, 24), (20.51, 24),               # boxes start at 5 / 5 / 6
    (15.0, 24), (14.99, 24), (14.5, 24),                # full from 0, full from 0, partial from -1
    (48.49, 24), (48.5, 24), (48.51, 24), (49.0, 24),   # the far edge in x: full, touching, partial
    (32, 20.49), (32, 20.5), (32, 20.51),
    (32, 15.0), (32, 14.99), (32, 14.5),                # the same in y
    (32, 32.49), (32, 32.5), (32, 32.51), (32, 33.0),
    (0.0, 0.0), (63.0, 47.0), (0.2, 47.3),              # corners
    (-20, 24), (32, -20), (100, 24), (32, 90),          # no overlap
    (78.4, 24), (78.6, 24),                             # the last overlapping column, none
    (1e300, 24), (32, -1e300),                          # beyond any int: no overlap
    (float("nan"), 24), (32, float("inf")), (float("-inf"), float("nan")),
]


@pytest.fixture(scope="module")
def cut_image():
    return np.random.default_rng(5).normal(100.0, 10.0, (48, 64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("size", [31, (30, 31)])
def test_cutouts_equal_the_restatement(mods, cut_image, dtype, size):
    B, _, _, S = mods
    img = cut_image.astype(dtype)
    want = ref.cutout_ref(img, CUT_POSITIONS, size)
    got = S.cutout_stamps(img, CUT_POSITIONS, size)
    assert got[0].dtype == dtype
    for g, w, what in zip(got, want, ("stamps", "boxes", "status")):
        assert same_bits(g, w), (what, np.argwhere(np.asarray(g) != np.asarray(w))[:5])
    st = got[2]
    if size == 31:  # the cases the positions were chosen for
        assert got[1][3:9, 0].tolist() == [5, 5, 6, 0, 0, -1]
        assert st[3:8].tolist() == [0] * 5 and st[8] == B.BSGP_STAMP_PARTIAL
        assert st[9:13].tolist() == [0, 0, B.BSGP_STAMP_PARTIAL, B.BSGP_STAMP_PARTIAL]
        assert st[16:23].tolist() == [0, 0, B.BSGP_STAMP_PARTIAL, 0, 0, B.BSGP_STAMP_PARTIAL,
                                      B.BSGP_STAMP_PARTIAL]
        assert st[23:26].tolist() == [B.BSGP_STAMP_PARTIAL] * 3
        assert st[26:30].tolist() == [B.BSGP_STAMP_NO_OVERLAP] * 4
        assert st[30:34].tolist() == [B.BSGP_STAMP_PARTIAL] + [B.BSGP_STAMP_NO_OVERLAP] * 3
        assert st[34:].tolist() == [B.BSGP_STAMP_BAD_POSITION] * 3
    # device in, device out: the same bits
    import torch
    dev = S.cutout_stamps(torch.from_numpy(img).cuda(),
                          torch.tensor(CUT_POSITIONS, dtype=torch.float64), size, device_out=True)
    assert all(t.is_cuda for t in dev) and same_bits(dev[0].cpu().numpy(), want[0])


def test_cutouts_integer_image_and_empty_list(mods, cut_image):
    _, _, _, S = mods
    img = cut_image.astype(np.int16)
    got = S.cutout_stamps(img, CUT_POSITIONS[:12], 31)
    want = ref.cutout_ref(img.astype(np.float64), CUT_POSITIONS[:12], 31)
    assert got[0].dtype == np.float64 and same_bits(got[0], want[0]) and same_bits(got[2], want[2])
    out, box, st = S.cutout_stamps(img, [], (30, 31))
    assert out.shape == (0, 30, 31) and box.shape == (0, 4) and st.shape == (0,)


def test_cutouts_reproduce_astropy_golden(mods):
    """astropy 4.3.1's own Cutout2D data (tests/golden/make_golden_io.py) at
    the golden boxes' centres, bit for bit."""
    _, _, _, S = mods
    g = golden("ref_cutouts.npz")
    b = g["boxes"].astype(np.float64)
    centres = np.stack(((b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2), axis=1)
    out, box, st = S.cutout_stamps(g["img"], centres, tuple(int(v) for v in g["shape"]))
    assert not st.any()
    np.testing.assert_array_equal(box, g["boxes"])
    assert same_bits(out, g["cutouts"])


# -------------------------------------------------------------------- select
def select_case():
    """n = 7 stars, K = 5 candidates: catalogue rows (cap 2: row 0 is label 1)
    with one case per star."""
    rng = np.random.default_rng(11)
    n, K = 7, 5

    def rows(m):
        c = np.zeros((m, 2, 8))
        c[..., 0] = rng.uniform(800.0, 1200.0, (m, 2))               # segment_flux
        c[..., 3:5] = rng.uniform(13.0, 17.0, (m, 2, 2))             # centroids
        sx, sy = rng.uniform(1.0, 3.0, (m, 2)), rng.uniform(1.0, 3.0, (m, 2))
        c[..., 5], c[..., 7] = sx, sy
        c[..., 6] = rng.uniform(-0.9, 0.9, (m, 2)) * np.sqrt(sx * sy)  # positive definite
        return c

    obs, res = rows(n), rows(n * K)
    obs[:, 0, 0] = 1000.0
    nl = np.ones(n * K, np.int32)
    f = res[:, 0, 0].reshape(n, K)  # a view: the restored fluxes of label 1
    assert np.shares_memory(f, res)
    f[0] = [900.0, 950.0, 990.0, 940.0, 930.0]       # a clear winner: candidate 2
    f[1] = [950.0, 980.0, 960.0, 980.0, 970.0]       # equal best scores: the first (1) wins
    f[2] = [np.nan, 960.0, 970.0, np.nan, 950.0]     # NaN scores never win: 2
    f[3] = [950.0, 999.0, 960.0, 970.0, 940.0]       # the best flux belongs to an undetected one
    nl[3 * K + 1] = 0
    f[4] = [950.0, 940.0, 985.0, 930.0, 920.0]       # two labels: label 1 is read
    nl[4 * K + 2] = 2
    res[4 * K + 2, 1, 0] = 5000.0
    nl[5 * K:6 * K] = 0                              # nothing detected: best -1, NaN row
    f[6] = [1100.0, 1300.0, 1200.0, 1300.0, 900.0]   # negative scores: the first 1300 (1)
    iters = rng.integers(5, 400, n * K).astype(np.int32)
    return n, K, nl, res, obs, iters


def check_select(B, S, seg, nl, res, obs, iters, K, want_best):
    want = ref.select_ref(nl, res, obs, iters, K)
    got = S.stamp_select(nl, res, obs, iters, K)
    assert got[1].tolist() == want[1].tolist() == want_best
    for g, w, what in zip(got, want, ("scores", "best", "rows", "num_iters", "status")):
        assert np.asarray(g).dtype == w.dtype, what
        np.testing.assert_array_equal(g, w, err_msg=what)  # NaN equals NaN, everything else exact
    # the two shape ratios against shape_columns on the host, bit for bit
    # (on whole columns, as the catalogue calls it)
    rows = got[2]
    so = seg.shape_columns(obs[:, 0, 5], obs[:, 0, 6], obs[:, 0, 7])
    sr = seg.shape_columns(res[:, 0, 5], res[:, 0, 6], res[:, 0, 7])
    for s, b in enumerate(want_best):
        if got[4][s]:
            assert np.isnan(rows[s, [1, 2, 3, 4, 8, 9, 10]]).all() and got[3][s] == -1
            continue
        i = s * K + b
        assert same_bits(rows[s, 3], sr["fwhm"][i] / so["fwhm"][s])
        assert same_bits(rows[s, 4], sr["ellipticity"][i] / so["ellipticity"][s])
        assert same_bits(rows[s, 7], so["fwhm"][s]) and same_bits(rows[s, 10], sr["fwhm"][i])
        assert got[3][s] == iters[i]
    return got


def test_select_equals_the_restatement(mods):
    B, _, seg, S = mods
    n, K, nl, res, obs, iters = select_case()
    got = check_select(B, S, seg, nl, res, obs, iters, K, [2, 1, 2, 3, 2, -1, 1])
    assert got[4].tolist() == [0, 0, 0, 0, 0, B.BSGP_STAMP_NO_CANDIDATE, 0]
    assert np.isinf(got[0][3, 1]) and np.isnan(got[0][2, 0]) and np.isinf(got[0][5]).all()


def test_select_shape_columns_bit_for_bit_on_many_rows(mods):
    """4096 stars x 2 candidates of random covariances: every row equals the
    restatement, so the device's square roots and divisions round as numpy's
    do on whole columns (the seven hand-made stars of the tests above would
    not show a rounding that differs once in a thousand rows)."""
    _, _, _, S = mods
    rng = np.random.default_rng(7)
    n, K = 4096, 2
    res, obs = rng.uniform(0.5, 4.0, (n * K, 1, 8)), rng.uniform(0.5, 4.0, (n, 1, 8))
    for c in (res, obs):
        c[..., 6] = rng.uniform(-0.95, 0.95, c.shape[:2]) * np.sqrt(c[..., 5] * c[..., 7])
    nl = np.ones(n * K, np.int32)
    it = rng.integers(1, 500, n * K).astype(np.int32)
    got, want = S.stamp_select(nl, res, obs, it, K), ref.select_ref(nl, res, obs, it, K)
    for g, w, what in zip(got, want, ("scores", "best", "rows", "num_iters", "status")):
        np.testing.assert_array_equal(g, w, err_msg=what)
    assert same_bits(got[2], want[2])


def test_select_one_candidate_is_the_kl_branch(mods):
    """K = 1: no search.  The restoration is the result whatever its score; one
    without a detection is a status bit."""
    B, _, seg, S = mods
    n, K, nl, res, obs, iters = select_case()
    nl1, res1, it1 = nl[::K].copy(), res[::K].copy(), iters[::K].copy()
    nl1[1], nl1[3] = 0, 2
    got = check_select(B, S, seg, nl1, res1, obs, it1, 1, [0] * n)
    assert got[4].tolist() == [0, B.BSGP_STAMP_RESTORED_NO_SOURCE, 0, 0, 0,
                               B.BSGP_STAMP_RESTORED_NO_SOURCE, 0]
    assert np.isnan(got[0][2, 0]) and np.isnan(got[2][2, 2]) and got[2][2, 3] > 0  # a NaN flux row


# -------------------------------------------------------------------- driver
# (x, y) of the stars of the 96 x 96 field, their peak values, and the
# positions handed to the driver
STARS = [(30.3, 28.7, 4000.0), (64.6, 30.2, 2500.0), (47.4, 66.5, 6000.0),  # isolated, interior
         (70.4, 6.3, 3000.0),                                               # 10 px from a border
         (76.0, 72.0, 3000.0), (80.0, 72.0, 2600.0)]                        # 4 px apart
POSITIONS = [(30.3, 28.7), (70.4, 6.3), (64.6, 30.2), (76.0, 72.0), (20.0, 78.0), (47.4, 66.5)]
ISOLATED = [0, 2, 5]
SOLVER_KW = dict(gamma=1e-4, beta=0.4, alpha_min=1e-5, alpha_max=1e5, alpha=10.0, M_alpha=3, tau=0.5,
                 M=1, max_projs=1000, proj_type=1, init_recon=2, stop_criterion=3,
                 ccd_sat_level=65000, scale_data=True, use_original_SGP_Afunction=True)
BETA_KW = dict(lr=1e-3, lr_exp_param=0.1, schedule_lr=True, adapt_beta=True)
SOURCE_KW = dict(n_pixels=5, deblend=True, localbkg_width=5, device_out=True)


@pytest.fixture(scope="module")
def field():
    """A flat sky of 200 with fixed-seed noise (sigma 4) and Gaussian stars of
    FWHM 3 px at sub-pixel centres, float32; the 31 x 31 golden PSF."""
    import fits_io
    _, psf = fits_io.read_fits(os.path.join(GOLDEN, "psfccfbrd210048_1_1_img.fits"))
    yy, xx = np.mgrid[:96, :96].astype(np.float64)
    img = 200.0 + np.random.default_rng(2024).normal(0.0, 4.0, (96, 96))
    sig = 3.0 / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    for x, y, peak in STARS:
        img += peak * np.exp(-0.5 * ((xx - x) ** 2 + (yy - y) ** 2) / sig ** 2)
    return img.astype(np.float32), np.asarray(psf)


def chain(mods, img, psf, use_betadiv):
    """The driver's chain from the public calls, the choice made on the host."""
    B, sgp, seg, S = mods
    stamps, _, st = S.cutout_stamps(img, POSITIONS, 31)
    status = st.astype(np.int32)
    full = np.flatnonzero(st == 0)
    cat_o, bkg_o = seg.source_info(stamps[full], (5, 5), **SOURCE_KW)
    nl = np.asarray(cat_o.nlabels)
    flux = np.array([f[0] if len(f) else np.nan for f in cat_o.segment_flux])
    status[full[nl == 0]] |= B.BSGP_STAMP_NO_SOURCE
    status[full[nl > 1]] |= B.BSGP_STAMP_MULTI_SOURCE
    status[full[(nl == 1) & ~(flux > 0)]] |= B.BSGP_STAMP_BAD_FLUX
    keep = np.flatnonzero((nl == 1) & (flux > 0))
    kept, nk = full[keep], len(keep)
    betas = sgp.app_beta_candidates() if use_betadiv else [np.nan]
    K = len(betas)
    gns = np.repeat(stamps[kept], K, axis=0)
    assert gns.dtype == np.float32
    bkgs, fl = np.repeat(bkg_o.background_median[keep], K), np.repeat(flux[keep], K)
    if use_betadiv:
        out = sgp.sgp_betaDiv_batch(gns, psf, bkgs, betaParams=np.tile(betas, nk), flux=fl,
                                    MAXIT=MAXIT, team=1, **SOLVER_KW, **BETA_KW)
    else:
        out = sgp.sgp_batch(gns, psf, bkgs, flux=fl, MAXIT=MAXIT, team=1, **SOLVER_KW)
    cat_r, _ = seg.source_info(out["x"], (5, 5), **SOURCE_KW)
    nlr = np.asarray(cat_r.nlabels)
    scores = np.full((nk, K), np.inf)
    for i in np.flatnonzero(nlr > 0):
        scores[i // K, i % K] = 1 - cat_r.segment_flux[i][0] / flux[keep[i // K]]
    best = [sgp.argmin_strict(row) if use_betadiv else 0 for row in scores]
    assert all(b is not None and nlr[s * K + b] > 0 for s, b in enumerate(best)), (best, nlr)
    win = np.arange(nk) * K + np.asarray(best)
    col = lambda cat, nm, idx: np.array([cat[nm][i][0] for i in idx])
    res = dict(ORIG_FLUX=flux[keep], RESTORED_FLUX=col(cat_r, "segment_flux", win))
    res["FLUX_FRACTIONAL_DIFFERENCE"] = 1 - res["RESTORED_FLUX"] / res["ORIG_FLUX"]
    res["FWHM_RATIO"] = col(cat_r, "fwhm", win) / col(cat_o, "fwhm", keep)
    res["ELLIPTICITY_RATIO"] = col(cat_r, "ellipticity", win) / col(cat_o, "ellipticity", keep)
    import torch
    met = S.stamp_metrics(
        cat_o.data[torch.from_numpy(keep).cuda()], cat_r.data[torch.from_numpy(win).cuda()],
        np.stack((col(cat_o, "xcentroid", keep), col(cat_o, "ycentroid", keep)), 1),
        np.stack((col(cat_r, "xcentroid", win), col(cat_r, "ycentroid", win)), 1),
        col(cat_o, "fwhm", keep), col(cat_r, "fwhm", win))
    res["WD_RADIAL_PROFILE_DISTANCE"] = met["wd"]
    res.update(NUM_ITERS=out["iters"][win], scores=scores, x=out["x"][win], best=np.asarray(best),
               beta_final=out["beta_final"][win], kept=kept, status=status, metrics=met,
               stamps=stamps[kept], bkg=bkg_o.background_median[keep], betas=betas)
    return res


@pytest.mark.parametrize("use_betadiv", [True, False])
def test_driver_equals_the_chain(mods, field, use_betadiv, monkeypatch):
    B, sgp, _, S = mods
    img, psf = field
    want = chain(mods, img, psf, use_betadiv)
    got = S.sgp_star_stamps(img, POSITIONS, psf, use_betadiv=use_betadiv, MAXIT=MAXIT, team=1)
    nk = len(got["kept"])
    print("kept", got["kept"], "status", got["status"], "best", got["best"], "iters",
          got["NUM_ITERS"], "ffd", got["FLUX_FRACTIONAL_DIFFERENCE"], "wd",
          got["WD_RADIAL_PROFILE_DISTANCE"])
    assert got["kept"].tolist() == want["kept"].tolist()
    assert got["status"].tolist() == want["status"].tolist()
    assert got["best"].tolist() == want["best"].tolist()
    assert got["NUM_ITERS"].tolist() == want["NUM_ITERS"].tolist()
    for k in ("ORIG_FLUX", "RESTORED_FLUX", "FLUX_FRACTIONAL_DIFFERENCE", "FWHM_RATIO",
              "ELLIPTICITY_RATIO", "WD_RADIAL_PROFILE_DISTANCE", "scores", "x"):
        assert same_bits(got[k], want[k]), k
    for k, v in want["metrics"].items():
        assert same_bits(got["metrics"][k], v), k
    if use_betadiv:
        assert same_bits(got["beta_final"], want["beta_final"])
        assert got["best_beta"].tolist() == [want["betas"][b] for b in want["best"]]
    else:
        assert np.isnan(got["beta_final"]).all() and np.isnan(got["best_beta"]).all()
        assert got["scores"].shape == (nk, 1)
    # one entry per kept star
    for k in S.RESULT_KEYS + ("best", "best_beta", "beta_final", "scores", "x", "solver_status"):
        assert len(got[k]) == nk, k
    assert got["EXEC_TIME"].dtype == np.float64 and (got["EXEC_TIME"] > 0).all()
    assert len(set(got["EXEC_TIME"].tolist())) == 1
    assert not got["solver_status"].any()
    # what the scene was built for
    st = got["status"]
    assert len(st) == len(POSITIONS) and set(ISOLATED) <= set(got["kept"].tolist())
    assert all(st[i] == 0 for i in got["kept"])
    assert st[1] == B.BSGP_STAMP_PARTIAL and st[4] == B.BSGP_STAMP_NO_SOURCE
    assert 3 in got["kept"] or st[3] in (B.BSGP_STAMP_MULTI_SOURCE, B.BSGP_STAMP_BAD_FLUX)
    # one kept star alone through the single-image drop-in with the winning
    # beta: the bar of tests/test_gpu_stamps.py's batch-versus-single checks
    # (the same bits at the same team size)
    monkeypatch.setattr(sgp, "TEAM_DEFAULT", 1)
    s = 1
    if use_betadiv:
        x1, it1, _, _, _ = sgp.sgp_betaDiv(want["stamps"][s], psf, want["bkg"][s],
                                           flux=want["ORIG_FLUX"][s], MAXIT=MAXIT,
                                           betaParam=float(got["best_beta"][s]), **SOLVER_KW,
                                           **BETA_KW)
    else:
        x1, it1, _, _, _ = sgp.sgp(want["stamps"][s], psf, want["bkg"][s],
                                   flux=want["ORIG_FLUX"][s], MAXIT=MAXIT, **SOLVER_KW)
    assert it1 == got["NUM_ITERS"][s]
    np.testing.assert_array_equal(x1, got["x"][s])


def test_driver_bad_input_launches_no_solve(mods, field, monkeypatch):
    """No position, or none that survives the cutouts and the selection: empty
    arrays and a full status, and the solver is never called."""
    B, sgp, _, S = mods
    img, psf = field

    def no_solve(*a, **k):
        raise AssertionError("a solve was launched")

    monkeypatch.setattr(sgp, "sgp_betaDiv_batch", no_solve)
    monkeypatch.setattr(sgp, "sgp_batch", no_solve)
    cases = [([], []),
             ([(3.0, 50.0), (float("nan"), 1.0), (500.0, 2.0)],
              [B.BSGP_STAMP_PARTIAL, B.BSGP_STAMP_BAD_POSITION, B.BSGP_STAMP_NO_OVERLAP]),
             ([(20.0, 78.0), (3.0, 50.0)], [B.BSGP_STAMP_NO_SOURCE, B.BSGP_STAMP_PARTIAL])]
    for pos, want in cases:
        for use_betadiv in (True, False):
            got = S.sgp_star_stamps(img, pos, psf, use_betadiv=use_betadiv, MAXIT=MAXIT)
            assert got["status"].tolist() == want and got["status"].dtype == np.int32
            K = 5 if use_betadiv else 1
            for k in S.RESULT_KEYS + ("kept", "best", "best_beta", "beta_final"):
                assert got[k].shape == (0,), k
            assert got["scores"].shape == (0, K) and got["x"].shape == (0, 31, 31)
            assert got["metrics"] is None
