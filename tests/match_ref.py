"""numpy restatement of the catalogue cross-match (include/bsgp.h and DESIGN
§3.10, M1 to M5): the greedy symmetric best match within ``max_sep``, as the
sorted walk that defines it (:func:`match_greedy`) and by rounds, as the
kernels compute it (:func:`match_rounds`, which also counts the rounds).

Every operation is numpy's float64 one, rounded once: ``dx * dx + dy * dy`` is
two products and a sum, ``np.sqrt`` is correctly rounded.  The candidates are
gathered in row chunks, so that two catalogues of thousands of rows need no
N x M matrix at once."""
import csv

import numpy as np

NONFINITE, OVER_CAP = 1, 2
# per catalogue, what tests/golden/match_cases.npz keeps of the reference's CSVs
CAT_COLUMNS = ("label", "xcentroid", "ycentroid", "segment_flux", "fwhm", "ellipticity")


def read_csv(path, columns, suffix=""):
    """The named columns (``name + suffix`` in the file) of a reference table,
    ``label`` as int64 and the others as float64, and ``Separation`` when the
    table has it."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for nm in columns:
        v = [r[nm + suffix] for r in rows]
        out[nm] = np.array(v, dtype=np.int64) if nm == "label" else np.array(v, dtype=np.float64)
    if rows and "Separation" in rows[0] and suffix:
        out["Separation"] = np.array([r["Separation"] for r in rows], dtype=np.float64)
    return out


def take_part(x, y, n=None, valid=None):
    """M1: (coordinates with NaN on every row that takes no part, status).
    The arrays' length is the cap; ``n`` may exceed it."""
    x, y = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
    cap = len(x)
    n = cap if n is None else int(n)
    status = OVER_CAP if n > cap else 0
    ok = np.arange(cap) < max(0, min(n, cap))
    if valid is not None:
        ok &= np.asarray(valid) > 0
    bad = ok & ~(np.isfinite(x) & np.isfinite(y))
    if bad.any():
        status |= NONFINITE
    ok &= ~bad
    x[~ok], y[~ok] = np.nan, np.nan
    return x, y, status


def candidates(x1, y1, x2, y2, max_sep, chunk=512):
    """M2: (i, j, d2) of every candidate, rows that take no part being NaN."""
    ii, jj, dd = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(x1), chunk):
            dx = x1[s:s + chunk, None] - x2[None, :]
            dy = y1[s:s + chunk, None] - y2[None, :]
            d2 = dx * dx + dy * dy
            i, j = np.nonzero((np.sqrt(d2) <= max_sep) & np.isfinite(d2))
            ii.append(i + s), jj.append(j), dd.append(d2[i, j])
    return (np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64),
            np.concatenate(dd)) if ii else (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))


def _result(n1, n2, pairs, d2, status):
    m1, m2 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)
    sep = np.full(n1, np.nan)
    for (i, j), d in zip(pairs, d2):
        m1[i], m2[j], sep[i] = j, i, np.sqrt(d)
    return dict(match1=m1, match2=m2, sep1=sep, npairs=len(pairs), status=status)


def _prepare(x1, y1, x2, y2, max_sep, n1, n2, valid1, valid2):
    x1, y1, s1 = take_part(x1, y1, n1, valid1)
    x2, y2, s2 = take_part(x2, y2, n2, valid2)
    return len(x1), len(x2), candidates(x1, y1, x2, y2, float(max_sep)), s1 | s2


def match_greedy(x1, y1, x2, y2, max_sep, n1=None, n2=None, valid1=None, valid2=None):
    """M3 and M4 as they are stated: the candidates sorted by (d2, i, j), a
    pair accepted iff neither row is taken.  M5's outputs for one image."""
    c1, c2, (i, j, d2), status = _prepare(x1, y1, x2, y2, max_sep, n1, n2, valid1, valid2)
    order = np.lexsort((j, i, d2))
    t1, t2 = np.zeros(c1, bool), np.zeros(c2, bool)
    pairs, dd = [], []
    for k in order:
        if not t1[i[k]] and not t2[j[k]]:
            t1[i[k]] = t2[j[k]] = True
            pairs.append((i[k], j[k])), dd.append(d2[k])
    return _result(c1, c2, pairs, dd, status)


def match_rounds(x1, y1, x2, y2, max_sep, n1=None, n2=None, valid1=None, valid2=None):
    """M4 by rounds: every untaken row of either catalogue picks its best
    untaken candidate, (d2, j) from catalogue 1's side and (d2, i) from
    catalogue 2's; mutual picks are accepted; a round that accepts nothing ends
    it.  Also returns ``rounds``, the accepting rounds, and ``accepted``, the
    pairs each of them took."""
    c1, c2, (i, j, d2), status = _prepare(x1, y1, x2, y2, max_sep, n1, n2, valid1, valid2)
    pairs, dd, accepted = [], [], []
    while len(i):
        o1 = np.lexsort((j, d2, i))  # per i: its best first
        first1 = o1[np.r_[True, i[o1][1:] != i[o1][:-1]]]
        o2 = np.lexsort((i, d2, j))
        first2 = o2[np.r_[True, j[o2][1:] != j[o2][:-1]]]
        mutual = np.intersect1d(first1, first2)
        if not len(mutual):
            break
        accepted.append(len(mutual))
        pairs += list(zip(i[mutual], j[mutual]))
        dd += list(d2[mutual])
        free = ~np.isin(i, i[mutual]) & ~np.isin(j, j[mutual])
        i, j, d2 = i[free], j[free], d2[free]
    out = _result(c1, c2, pairs, dd, status)
    out["rounds"], out["accepted"] = len(accepted), accepted
    return out


def pairs_of(res):
    """(idx1, idx2, separation) ordered by idx1, as the published tables are."""
    idx1 = np.flatnonzero(res["match1"] >= 0)
    return idx1, res["match1"][idx1].astype(np.int64), res["sep1"][idx1]


def check_abi_errors(_bsgp):
    """Every error return of bsgp_match_catalogs, with pointers that are never
    followed: the checks come first."""
    L = _bsgp.lib()
    p = 8

    def call(x1=p, y2=p, stride1=1, stride2=1, valid1=None, vstride1=1, vstride2=1, valid2=None,
             cap1=4, cap2=4, B=1, max_sep=1.1, path=0, match1=p, sep1=p, status=p):
        return L.bsgp_match_catalogs(x1, p, stride1, valid1, vstride1, cap1, None, p, y2, stride2,
                                     valid2, vstride2, cap2, None, B, max_sep, path, match1, p, sep1,
                                     p, status, None)

    for kw, word in ((dict(max_sep=-1.0), b"max_sep"), (dict(max_sep=float("nan")), b"max_sep"),
                     (dict(max_sep=float("inf")), b"max_sep"), (dict(cap1=0), b"cap"),
                     (dict(cap2=-3), b"cap"), (dict(B=-1), b"B"), (dict(stride1=0), b"stride"),
                     (dict(stride2=-8), b"stride"), (dict(valid1=p, vstride1=0), b"vstride"),
                     (dict(valid2=p, vstride2=0), b"vstride"), (dict(path=3), b"path"),
                     (dict(path=-1), b"path"), (dict(x1=None), b"x1"), (dict(y2=None), b"y2"),
                     (dict(match1=None), b"match1_out"), (dict(sep1=None), b"sep1_out"),
                     (dict(status=None), b"status_out")):
        assert call(**kw) == _bsgp.BSGP_ERR_ARG and word in L.bsgp_last_error(), kw
    for kw, word in ((dict(cap1=16385), b"16384"), (dict(cap2=16385, path=2), b"16384"),
                     (dict(cap1=4000, cap2=97, path=1), b"LDS"),
                     (dict(cap1=16384, cap2=1, path=1), b"LDS")):
        assert call(**kw) == _bsgp.BSGP_ERR_UNSUPPORTED and word in L.bsgp_last_error(), kw
    # no image: a no-op that follows no pointer, whatever the path
    for path in (0, 1, 2):
        assert L.bsgp_match_catalogs(None, None, 1, None, 1, 4, None, None, None, 1, None, 1, 4, None,
                                     0, 1.1, path, None, None, None, None, None, None) == 0
    # a vstride is not looked at without its valid array
    assert call(vstride1=0, B=0) == 0


def chain(n=40):
    """Points on a line with the gaps 1 + (2n - k) * 0.01, k = 0 .. 2n - 2,
    alternating between catalogues 1 and 2: at max_sep = 2 every gap is a
    candidate and each is smaller than the one before, so only the last pair is
    mutual, and after it the one before: n accepting rounds of one pair each."""
    gaps = 1.0 + (2 * n - np.arange(2 * n - 1)) * 0.01
    pos = np.concatenate([[0.0], np.cumsum(gaps)])
    return pos[0::2].copy(), np.zeros(n), pos[1::2].copy(), np.zeros(n)
