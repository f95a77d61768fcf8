"""CPU-side checks of the background-matched co-add: the
pair geometry of ``subdivisions.tile_pairs`` against a double loop, the claim
the device solver rests on -- reproject's shuffled gradient descent converges
to the least-squares solution whatever its shuffles -- on the numpy
restatement (tests/coadd_ref.py), and the unchanged default of coadd_tiles."""
import inspect

import numpy as np
import pytest

import coadd_ref
import subdivisions

GRIDS = [((100, 130), (45, 39), 7), ((64, 64), (48, 48), 8), ((120, 120), (32, 32), 6)]
TWO_COMPONENTS = np.asarray([[0, 0, 10, 10], [6, 0, 16, 10], [6, 7, 16, 17],   # all overlap
                             [40, 40, 50, 50], [49, 49, 59, 59],               # a 1-pixel overlap
                             [100, 0, 110, 10]], dtype=np.int32)               # alone


def _brute_adjacency(n, pr):
    rows = [[] for _ in range(n)]
    for p, (i, j) in enumerate(pr):
        rows[i].append((j, p, 1))
        rows[j].append((i, p, -1))
    return [sorted(r) for r in rows]


def _check_geometry(boxes):
    g = subdivisions.tile_pairs(boxes)
    n = len(boxes)
    pr, rects = coadd_ref.pairs(boxes)
    assert g.n == n
    np.testing.assert_array_equal(g.pairs, pr)
    np.testing.assert_array_equal(g.rects, rects)
    assert g.pairs.dtype == np.int32 and g.row_ptr.dtype == np.int32
    assert g.row_ptr[0] == 0 and g.row_ptr[-1] == 2 * len(pr) == len(g.nbr)
    for i, row in enumerate(_brute_adjacency(n, pr)):
        lo, hi = g.row_ptr[i], g.row_ptr[i + 1]
        got = list(zip(g.nbr[lo:hi].tolist(), g.nbr_pair[lo:hi].tolist(),
                       g.nbr_sign[lo:hi].tolist()))
        assert got == row, (i, got, row)
    comp, ncomp = coadd_ref.components(n, pr)
    np.testing.assert_array_equal(g.component, comp)
    assert g.ncomp == ncomp
    return g


@pytest.mark.parametrize("shape,tile,overlap", GRIDS)
def test_tile_pairs_on_grids(shape, tile, overlap):
    boxes = subdivisions.subdivision_boxes(shape, tile, overlap)
    g = _check_geometry(boxes)
    assert g.ncomp == 1
    if shape == (100, 130):  # the counts the GPU tests rest on
        cnt = (g.rects[:, 2] - g.rects[:, 0]) * (g.rects[:, 3] - g.rects[:, 1])
        assert (len(boxes), len(g.pairs)) == (12, 29)
        assert (cnt.min(), cnt.max(), int((cnt % 2).sum())) == (49, 1092, 14)


def test_tile_pairs_without_overlap_and_two_components():
    boxes = subdivisions.subdivision_boxes((90, 120), (30, 30), 0)
    g = _check_geometry(boxes)
    assert len(g.pairs) == 0 and g.ncomp == len(boxes) == 12
    assert g.pairs.shape == (0, 2) and g.rects.shape == (0, 4)
    g = _check_geometry(TWO_COMPONENTS)
    assert g.pairs.tolist() == [[0, 1], [0, 2], [1, 2], [3, 4]]
    assert g.rects[3].tolist() == [49, 49, 50, 50]
    assert g.component.tolist() == [0, 0, 0, 1, 1, 2] and g.ncomp == 3
    g = _check_geometry(np.asarray([[0, 0, 4, 4]], np.int32))
    assert g.ncomp == 1 and g.row_ptr.tolist() == [0, 0]


def _tiles(boxes, tile, seed, integer=False):
    rng = np.random.default_rng(seed)
    H, W = int(boxes[:, 3].max()), int(boxes[:, 2].max())
    yy, xx = np.mgrid[:H, :W]
    field = 50 + 0.1 * xx + 0.05 * yy + 3 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
    t = np.stack([field[y0:y1, x0:x1] for x0, y0, x1, y1 in boxes])
    t = t + rng.normal(0, 5, len(boxes))[:, None, None] + rng.normal(0, 0.3, t.shape)
    return np.rint(t) if integer else t


@pytest.mark.parametrize("shape,tile,overlap", [g for g in GRIDS if g[0] != (120, 120)]
                         + [((160, 160), (48, 48), 8)])
def test_shuffled_sgd_lands_on_the_least_squares_solution(shape, tile, overlap):
    """4, 12 and 16 tiles, three shuffle seeds: within reproject's own
    convergence threshold, 1e-10 * max|c|, of lstsq on the Laplacian."""
    boxes = subdivisions.subdivision_boxes(shape, tile, overlap)
    n = len(boxes)
    assert n in (4, 12, 16)
    pr, rects = coadd_ref.pairs(boxes)
    off, st = coadd_ref.offsets(_tiles(boxes, tile, 1), boxes, pr, rects)
    assert not st.any() and np.all(np.isfinite(off))
    c, st = coadd_ref.corrections(n, pr, off)
    assert not st.any() and abs(c.mean()) <= 4 * np.finfo(float).eps * np.abs(c).max()
    for seed in (0, 1, 2):
        cs, sweeps = coadd_ref.sgd(n, pr, off, seed)
        assert sweeps < 200, sweeps
        err = np.abs(cs - c).max() / np.abs(c).max()
        print(f"n={n} seed={seed}: {sweeps} sweeps, |sgd - lstsq| / max|c| = {err:.2e}")
        assert err <= 1e-10, (seed, err)


def test_reference_solution_properties():
    """The restated B3: zero mean per component, 0 and the bit for the tile
    alone, background_reference (index 0 too) zeroes that tile, and the matched
    mosaic of noise-free tiles has no seams."""
    b = TWO_COMPONENTS
    t = _tiles(b, (10, 10), 3)
    mean, foot, c, off, pr, st = coadd_ref.matched(t, b, (60, 110))
    assert st.tolist() == [0, 0, 0, 0, 0, coadd_ref.ISOLATED] and c[5] == 0.0
    assert abs(c[:3].sum()) < 1e-13 and abs(c[3:5].sum()) < 1e-13
    c0 = coadd_ref.corrections(len(b), pr, off, background_reference=0)[0]
    assert c0[0] == 0.0
    np.testing.assert_allclose(c0[:3] - c0[0], c[:3] - c[0], atol=1e-13)
    assert foot.max() == 3 and foot[30, 105] == 0 and mean[30, 105] == 0.0


def test_coadd_tiles_defaults_to_no_matching():
    p = inspect.signature(subdivisions.coadd_tiles).parameters
    assert list(p)[:3] == ["tiles", "boxes", "shape"]
    assert p["match_background"].default is False and p["background_reference"].default is None
    for fn in (subdivisions.sgp_subdivisions, subdivisions.sgp_subdivisions_multistart):
        q = inspect.signature(fn).parameters
        assert q["match_background"].default is False
        assert q["background_reference"].default is None


def test_entry_points_registered():
    import _bsgp
    for name in ("bsgp_tile_offsets", "bsgp_tile_corrections", "bsgp_coadd_tiles_matched"):
        assert name in _bsgp.EXPORTED and hasattr(_bsgp.lib(), name)
    assert (_bsgp.BSGP_COADD_NONFINITE, _bsgp.BSGP_COADD_ISOLATED,
            _bsgp.BSGP_COADD_NOT_CONVERGED) == (coadd_ref.NONFINITE, coadd_ref.ISOLATED,
                                                coadd_ref.NOT_CONVERGED) == (1, 2, 4)
    assert _bsgp.lib().bsgp_abi_version() == 3
