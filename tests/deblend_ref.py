"""Restatement of the device deblending (beta-sgp_amd/segmentation.py
``deblend_sources``) in numpy and
``scipy.ndimage.label``: what tests/golden/make_golden_deblend.py writes its
expected label images with, and what the tests use where no fixture exists.

The flood is a parameter.  The default, :func:`flood_serial`, is the serial
flood of D5 with the device's tie rule (equal values: the smaller index first).
The generator passes ``skimage.segmentation.watershed``, which breaks ties by
insertion age; it asserts that its cases are tie-free and that both floods
agree on them.
"""
import heapq

import numpy as np
from scipy import ndimage

MARGIN = 1e-9


class MarginError(AssertionError):
    pass


def flood_serial(neg, markers, mask, connectivity):
    """watershed(neg, markers, mask=mask, connectivity=structure) by D5: a
    priority queue keyed by (neg, linear index) holds the marker pixels; the
    smallest key is popped and each unlabelled neighbour inside the mask takes
    the popped pixel's label on discovery and is entered."""
    H, W = neg.shape
    out = np.where(mask, markers, 0).astype(np.int32)
    st = np.asarray(connectivity, bool)
    offs = [(dy - 1, dx - 1) for dy in range(3) for dx in range(3) if st[dy, dx] and (dy, dx) != (1, 1)]
    heap = [(neg[y, x], y * W + x) for y, x in zip(*np.nonzero(out))]
    heapq.heapify(heap)
    while heap:
        _, p = heapq.heappop(heap)
        y, x = divmod(p, W)
        for dy, dx in offs:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and mask[yy, xx] and out[yy, xx] == 0:
                out[yy, xx] = out[y, x]
                heapq.heappush(heap, (neg[yy, xx], yy * W + xx))
    return out


def structure(connectivity):
    return np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)


def thresholds(smin, smax, nlevels, mode):
    k = np.arange(1, nlevels + 1, dtype=np.float64)
    if mode == "exponential" and smin < 0:
        mode = "linear"
    if mode == "linear":
        return smin + (smax - smin) / (nlevels + 1) * k
    m = smin if smin != 0 else 0.01 * smax
    return m * (smax / m) ** (k / (nlevels + 1))


def deblend_parent(data, M, npixels, nlevels, contrast, mode, connectivity, stats, flood=flood_serial):
    """Children of the parent with pixel set M (bool image) as a list of bool
    images ordered by marker identity, or None where the parent stays."""
    st = structure(connectivity)
    v = data[M]
    smin, smax, ssum = v.min(), v.max(), v.sum()
    if smin == smax:
        return None
    s = np.sort(v)
    gap = np.min(np.diff(s) / np.maximum(np.abs(s[1:]), np.abs(s[:-1]))) if len(s) > 1 else np.inf
    stats["gap"] = min(stats["gap"], gap)
    regions = [M]
    for t in thresholds(smin, smax, nlevels, mode):
        stats["thr"] = min(stats["thr"], np.min(np.abs(v - t) / np.maximum(np.abs(v), abs(t))))
        lab, n = ndimage.label(M & (data > t), structure=st)
        if n == 0:
            continue
        areas = ndimage.sum(np.ones_like(lab), lab, np.arange(1, n + 1))
        kept = [lab == i for i in range(1, n + 1) if areas[i - 1] >= npixels]
        new = []
        for R in regions:
            inside = [c for c in kept if R[c].any()]
            assert all(R[c].all() for c in inside)
            if len(inside) >= 2:
                new.extend(inside)
                stats["splits"] += 1
            else:
                new.append(R)
        regions = new
    if len(regions) == 1 and regions[0] is M:
        return None
    regions.sort(key=lambda R: np.flatnonzero(R)[0])  # marker identity: first pixel in raster order
    markers = np.zeros(data.shape, dtype=np.int32)
    for i, R in enumerate(regions, start=1):
        markers[R] = i
    stats.setdefault("markers", []).append(markers.copy())
    while True:
        markers = flood(-data, markers, mask=M, connectivity=st)
        ids = np.unique(markers[markers != 0])
        frac = ndimage.sum(data, markers, ids) / ssum
        # with one child left the outcome no longer depends on its fraction
        if contrast > 0 and len(ids) > 1:
            stats["frac"] = min(stats["frac"], np.min(np.abs(frac - contrast)) / contrast)
        low = np.sort(frac[frac < contrast])
        if len(low) > 1 and len(ids) > 1:
            stats["frac"] = min(stats["frac"], np.min(np.diff(low) / np.abs(low[1:])))
        if not (frac < contrast).any():
            break
        markers[markers == ids[np.argmin(frac)]] = 0
        stats["removals"] += 1
        if len(ids) == 1:
            break
    ids = np.unique(markers[markers != 0])
    if len(ids) < 2:
        return None
    return [markers == i for i in ids]


def deblend(data, seg, npixels, labels=None, nlevels=32, contrast=0.001, mode="exponential",
            connectivity=8, flood=flood_serial, margin=MARGIN):
    """(deblended label image, parent of every output label 0..n, statistics).
    Raises MarginError where a tie-freeness margin (make_golden_deblend.py's
    three conditions) is below ``margin``; ``margin=0`` for inputs with ties."""
    data = np.asarray(data, dtype=np.float64)
    seg = np.asarray(seg).astype(np.int32)
    stats = dict(gap=np.inf, thr=np.inf, frac=np.inf, splits=0, removals=0, nsplit=0, nchildren=0)
    n = int(seg.max())
    chosen = range(1, n + 1) if labels is None else labels
    kids = {}
    for l in range(1, n + 1):
        M = seg == l
        if l not in chosen or M.sum() < 2 * npixels:
            continue
        c = deblend_parent(data, M, npixels, nlevels, contrast, mode, connectivity, stats, flood)
        if c is not None:
            kids[l] = c
    out = np.zeros_like(seg)
    parent = [0]
    for l in range(1, n + 1):
        if l not in kids and (seg == l).any():
            out[seg == l] = len(parent)
            parent.append(l)
    for l in sorted(kids):
        for c in kids[l]:
            out[c] = len(parent)
            parent.append(l)
    stats["nsplit"], stats["nchildren"] = len(kids), sum(len(c) for c in kids.values())
    for k in ("gap", "thr", "frac"):
        if stats[k] < margin:
            raise MarginError(f"{k} margin {stats[k]:.2e}")
    return out, np.array(parent, dtype=np.int32), stats
