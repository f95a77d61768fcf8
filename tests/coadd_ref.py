"""numpy restatement of the background-matched co-add:
what ``reproject_and_coadd(..., match_background=True)`` computes for tiles on
one pixel grid (restoration/utils.py:392-397), written from that description.

B1 ``pairs``         every i < j whose boxes intersect, ordered by (i, j)
B2 ``offsets``       numpy.median of tile_i - tile_j over the intersection
B3 ``corrections``   the minimum-norm least-squares solution of
                     c_i - c_j = O_ij (numpy.linalg.lstsq on the graph
                     Laplacian), zero mean in every connected component;
   ``sgd``           the solver reproject runs instead, restated: a per-row
                     update in shuffled order, re-centred every sweep, which
                     has that solution as its fixed point
B4 ``coadd``         mean of (tile - c) in tile order, and the footprint
"""
import numpy as np

NONFINITE, ISOLATED, NOT_CONVERGED = 1, 2, 4  # BSGP_COADD_* (include/bsgp.h)


def pairs(boxes):
    """B1 by the double loop: ([P, 2] pairs, [P, 4] xyxy intersections)."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    pr, rc = [], []
    for i in range(len(b)):
        for j in range(i + 1, len(b)):
            x0, y0 = max(b[i, 0], b[j, 0]), max(b[i, 1], b[j, 1])
            x1, y1 = min(b[i, 2], b[j, 2]), min(b[i, 3], b[j, 3])
            if x1 > x0 and y1 > y0:
                pr.append((i, j))
                rc.append((x0, y0, x1, y1))
    return (np.asarray(pr, dtype=np.int32).reshape(-1, 2),
            np.asarray(rc, dtype=np.int32).reshape(-1, 4))


def components(n, pr):
    """Connected component of every tile, numbered by their first tile, and their count."""
    comp = np.arange(n)
    for _ in range(n):  # label propagation to the minimum: at most n sweeps
        old = comp.copy()
        for i, j in pr:
            comp[i] = comp[j] = min(comp[i], comp[j])
        if np.array_equal(old, comp):
            break
    _, comp = np.unique(comp, return_inverse=True)
    return comp.astype(np.int32), int(comp.max()) + 1 if n else 0


def offsets(tiles, boxes, pr=None, rects=None):
    """B2: (offsets [P], status [n]); a pair with a non-finite difference is NaN."""
    t = np.asarray(tiles, dtype=np.float64)
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    if pr is None:
        pr, rects = pairs(b)
    off = np.empty(len(pr))
    status = np.zeros(len(b), np.int32)
    for p, ((i, j), (x0, y0, x1, y1)) in enumerate(zip(pr, rects)):
        a = t[i, y0 - b[i, 1]:y1 - b[i, 1], x0 - b[i, 0]:x1 - b[i, 0]]
        c = t[j, y0 - b[j, 1]:y1 - b[j, 1], x0 - b[j, 0]:x1 - b[j, 0]]
        d = a - c
        if np.all(np.isfinite(d)):
            off[p] = np.median(d)
        else:
            off[p] = np.nan
            status[i] |= NONFINITE
            status[j] |= NONFINITE
    return off, status


def laplacian(n, pr, off):
    """L and b of L c = b over the pairs with a finite offset."""
    L = np.zeros((n, n))
    rhs = np.zeros(n)
    for (i, j), o in zip(pr, off):
        if not np.isfinite(o):
            continue
        L[i, i] += 1
        L[j, j] += 1
        L[i, j] -= 1
        L[j, i] -= 1
        rhs[i] += o
        rhs[j] -= o
    return L, rhs


def corrections(n, pr, off, background_reference=None):
    """B3: (c [n], status [n]).  lstsq's minimum-norm solution is zero-mean in
    every component (the null space of L is spanned by their indicators)."""
    L, rhs = laplacian(n, pr, off)
    c = np.linalg.lstsq(L, rhs, rcond=None)[0] if n else np.zeros(0)
    status = np.zeros(n, np.int32)
    iso = np.diag(L) == 0
    status[iso] |= ISOLATED
    c[iso] = 0.0
    if background_reference is not None:
        c = c - c[background_reference]
    return c, status


def sgd(n, pr, off, seed, eta_initial=1.0, eta_half_life=100.0, rtol=1e-10, atol=0.0,
        max_sweeps=100000):
    """B3 by reproject's solver, restated: every sweep visits the rows in a
    shuffled order (a seeded RandomState), row i moving by eta times the mean
    over its neighbours of O_ij - (c_i - c_j); c is re-centred to zero mean
    after the sweep; eta halves every eta_half_life sweeps; the sweeps end when
    no correction moved by more than rtol * |c| + atol.
    Returns (c, sweeps).  For a connected graph."""
    rs = np.random.RandomState(seed)
    O = np.full((n, n), np.nan)
    for (i, j), o in zip(pr, off):
        O[i, j], O[j, i] = o, -o
    has = np.isfinite(O)
    c = np.zeros(n)
    for sweep in range(max_sweeps):
        eta = eta_initial * 0.5 ** (sweep / eta_half_life)
        old = c.copy()
        for i in rs.permutation(n):
            nb = has[i]
            if nb.any():
                c[i] += eta * np.mean(O[i, nb] - (c[i] - c[nb]))
        c -= c.mean()
        if np.all(np.abs(c - old) <= rtol * np.abs(c) + atol):
            return c, sweep + 1
    return c, max_sweeps


def coadd(tiles, boxes, shape, c=None):
    """B4: (mean, footprint); tiles summed in index order, c_t taken off each
    value before it is added; uncovered pixels are 0."""
    t = np.asarray(tiles, dtype=np.float64)
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    s = np.zeros(shape)
    cnt = np.zeros(shape)
    for k, (x0, y0, x1, y1) in enumerate(b):
        v = t[k, :y1 - y0, :x1 - x0]
        s[y0:y1, x0:x1] += v if c is None else v - c[k]
        cnt[y0:y1, x0:x1] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, s / cnt, 0.0)
    return mean, cnt


def matched(tiles, boxes, shape, background_reference=None):
    """B1-B4 in one call: (mean, footprint, c, offsets, pairs, status)."""
    pr, rects = pairs(boxes)
    off, st = offsets(tiles, boxes, pr, rects)
    c, st2 = corrections(len(np.asarray(boxes).reshape(-1, 4)), pr, off, background_reference)
    mean, foot = coadd(tiles, boxes, shape, c)
    return mean, foot, c, off, pr, st | st2
