"""Plain-numpy restatement of the local background of the source catalogue
(include/bsgp.h and DESIGN §3.8, L1 to L6): what
``SourceCatalog(..., localbkg_width=L)`` computes on the device.
tests/golden/make_golden_localbkg.py writes tests/golden/localbkg_cases.npz
with it and pins its clipping to ``astropy.stats.SigmaClip``; the published
catalogue tests/golden/SUBDIV_ORIGCAT.csv pins the conventions (L1, L2, L5).

Device and restatement select the same pixels (L2 is the same float64
comparisons), so the sorted values, both counts and the median are equal
exactly.  The mean and the standard deviation differ by summation order; the
bars below bound what that does to ``lb`` and to the corrected columns."""
import numpy as np

FEW, OVER_CAP = 1, 2
MAX_VALUES = 8192
U = 2.0 ** -53


def annulus(shape, box, width):
    """L1, L2 without the label and finiteness tests: the boolean mask of the
    rectangular annulus of the inclusive box (x0, x1, y0, y1)."""
    H, W = shape
    x0, x1, y0, y1 = (float(v) for v in box)
    cx, cy = (x0 + x1) / 2.0, (y0 + y1) / 2.0
    ix, iy = 0.75 * (x1 - x0 + 1.0), 0.75 * (y1 - y0 + 1.0)
    ox, oy = ix + width, iy + width
    dx, dy = np.abs(np.arange(W) - cx), np.abs(np.arange(H) - cy)
    return np.outer(dy < oy, dx < ox) & ~np.outer(dy < iy, dx < ix)


def values(data, labels, box, width):
    """L2: the float64 values of the annulus, sorted."""
    d = np.asarray(data)
    m = annulus(d.shape, box, width) & (np.asarray(labels) == 0)
    v = d[m].astype(np.float64)
    return np.sort(v[np.isfinite(v)])


def clip_sorted(s, sigma=3.0, maxiters=10):
    """L4 as the device runs it on the sorted values s: (lo, hi, iterations,
    median, mean, std, margin); margin is the smallest relative distance of a
    value to a clipping bound over the iterations (inf where std is 0)."""
    lo, hi, it, more, margin = 0, len(s), 0, maxiters > 0, np.inf
    while True:
        v, n = s[lo:hi], hi - lo
        med = v[n // 2] if n & 1 else (v[n // 2 - 1] + v[n // 2]) / 2.0
        mean = v.sum() / n
        sd = np.sqrt(((v - mean) ** 2).sum() / n)
        if not more:
            break
        lb, ub = med - sd * sigma, med + sd * sigma
        if sd > 0:
            dist = min(np.min(np.abs(v - lb)), np.min(np.abs(v - ub)))
            margin = min(margin, dist / max(abs(lb), abs(ub)))
        nlo, nhi = lo + np.searchsorted(v, lb, "left"), lo + np.searchsorted(v, ub, "right")
        it += 1
        if nhi <= nlo:
            return nlo, nlo, it, np.nan, np.nan, np.nan, margin
        changed = (nlo, nhi) != (lo, hi)
        lo, hi = int(nlo), int(nhi)
        if not changed:
            break
        more = it < maxiters
    return lo, hi, it, med, mean, sd, margin


def mode_estimate(mean, med, sd):
    """L5: SExtractor's mode."""
    if sd == 0:
        return mean
    if abs(mean - med) / sd < 0.3:
        return 2.5 * med - 1.5 * mean
    return med


def local_background(data, labels, boxes, areas, width, sigma=3.0, maxiters=10, min_pixels=10):
    """L1 to L5 for labels 1..n with inclusive boxes [n, 4] = (xmin, xmax, ymin,
    ymax) and areas [n].  Returns a dict of arrays over the labels: lb,
    ngather, nsurv, iters, bar (the derived bar of lb), margin (clipping),
    ratio (|mean - median| / std of the survivors, 0 where std is 0), branch
    (|ratio - 0.3|, inf where std is 0 or no estimate is made) and the int status (the OR of the FEW / OVER_CAP bits)."""
    n = len(areas)
    out = dict(lb=np.zeros(n), ngather=np.zeros(n, np.int32), nsurv=np.zeros(n, np.int32),
               iters=np.zeros(n, np.int32), bar=np.zeros(n), margin=np.full(n, np.inf),
               ratio=np.zeros(n), branch=np.full(n, np.inf))
    status = 0
    for l in range(n):
        if areas[l] <= 0:
            continue
        s = values(data, labels, boxes[l], width)
        out["ngather"][l] = len(s)
        if len(s) > MAX_VALUES:
            status |= OVER_CAP
            continue
        if len(s) < min_pixels:
            status |= FEW
            continue
        lo, hi, it, med, mean, sd, margin = clip_sorted(s, sigma, maxiters)
        out["lb"][l] = mode_estimate(mean, med, sd)
        out["nsurv"][l], out["iters"][l], out["margin"][l] = hi - lo, it, margin
        if sd > 0:
            out["ratio"][l] = abs(mean - med) / sd
            out["branch"][l] = abs(out["ratio"][l] - 0.3)
        # two summation orders of m terms differ by at most 2 m u sum|v|; the
        # mean divides that by m and rounds once more; lb = 2.5 med - 1.5 mean
        # scales it by 1.5 and rounds three times (bounded by 4 u (|med| + |mean|))
        m, sabs = hi - lo, np.abs(s[lo:hi]).sum()
        out["bar"][l] = 1.5 * (2 * m * U * sabs / m + U * abs(mean)) + 4 * U * (abs(med) + abs(mean))
    out["status"] = status
    return out


def corrected(cat, lb):
    """L6 on a catalogue of seg_ref.catalog: the three corrected columns."""
    area = cat["area"].astype(np.float64)
    return dict(segment_flux=cat["segment_flux"] - area * lb, min_value=cat["min_value"] - lb,
                max_value=cat["max_value"] - lb)


def column_bars(cat, lb, lb_bar, flux_bar):
    """The derived bars of the corrected columns: the bar of the uncorrected
    flux (seg_ref.column_bars), area times the bar of lb, and the roundings of
    the product and the difference."""
    area = cat["area"].astype(np.float64)
    flux = flux_bar + area * lb_bar + 4 * U * (np.abs(cat["segment_flux"]) + area * np.abs(lb))
    return dict(segment_flux=flux,
                min_value=lb_bar + 2 * U * (np.abs(cat["min_value"]) + np.abs(lb)),
                max_value=lb_bar + 2 * U * (np.abs(cat["max_value"]) + np.abs(lb)))


def read_published(path):
    """The columns of the published catalogue (a CSV that photutils' table
    wrote) the tests use, as a dict of float64 arrays."""
    with open(path) as f:
        head = f.readline().rstrip("\n").split(",")
        rows = [line.rstrip("\n").split(",") for line in f if line.strip()]
    want = ("bbox_xmin", "bbox_xmax", "bbox_ymin", "bbox_ymax", "area", "min_value", "max_value",
            "local_background", "segment_flux")
    return {k: np.array([float(r[head.index(k)]) for r in rows]) for k in want}


def match_rows(cat, pub):
    """Per row of the published catalogue the index of our segment with the
    same (bbox, area), or -1."""
    key = {}
    for i in range(len(cat["area"])):
        key.setdefault((int(cat["bbox_xmin"][i]), int(cat["bbox_xmax"][i]), int(cat["bbox_ymin"][i]),
                        int(cat["bbox_ymax"][i]), int(cat["area"][i])), i)
    return np.array([key.get((int(pub["bbox_xmin"][j]), int(pub["bbox_xmax"][j]),
                              int(pub["bbox_ymin"][j]), int(pub["bbox_ymax"][j]),
                              int(pub["area"][j])), -1) for j in range(len(pub["area"]))])


def check_against_published(cat, lb, corrected_flux, raw_min, pub):
    """The three assertions against the published catalogue, for the
    restatement's numbers and for the device's: at least 97 of the 103 rows
    match in (bbox, area); on those |lb - published| is at most twice the
    largest |raw minimum - (published min_value + local_background)|, the
    disagreement of the two background maps measured on the same rows; the sum
    of the corrected fluxes is within 5e-4 of the published sum.  Prints and
    returns the figures."""
    match = match_rows(cat, pub)
    ok = match >= 0
    m = match[ok]
    raw_gap = np.abs(raw_min[m] - (pub["min_value"][ok] + pub["local_background"][ok])).max()
    lb_gap = np.abs(lb[m] - pub["local_background"][ok]).max()
    psum = pub["segment_flux"].sum()
    rel = abs(np.sum(corrected_flux) - psum) / psum
    print(f"matched {ok.sum()} of {len(ok)}; max |lb - published| {lb_gap:.4f} against background-map "
          f"disagreement {raw_gap:.4f}; sum {np.sum(corrected_flux):.2f} against {psum:.2f} "
          f"(rel {rel:.2e})")
    assert ok.sum() >= 97, ok.sum()
    assert lb_gap <= 2 * raw_gap, (lb_gap, raw_gap)
    assert rel <= 5e-4, rel
    return dict(matched=int(ok.sum()), lb_gap=lb_gap, raw_gap=raw_gap, rel=rel)


def published_frame(fx, img):
    """The published frame as the fixture's generator saw it: (sub, labels,
    catalogue of seg_ref.catalog, boxes [n, 4]) from the float32 frame img, the
    fixture's two filtered meshes (zoomed by tests/bkg_ref.zoom) and its labels."""
    import bkg_ref
    import seg_ref
    bkg = bkg_ref.zoom(fx["pub_bkg_mesh"], (60, 60), img.shape)
    sub = img.astype(np.float64) - bkg
    labels = fx["pub_labels"].astype(np.int32)
    cat = seg_ref.catalog(sub, labels)
    box = np.stack([cat["bbox_xmin"], cat["bbox_xmax"], cat["bbox_ymin"], cat["bbox_ymax"]], 1)
    return sub, labels, cat, box
