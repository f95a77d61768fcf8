"""Generate tests/golden/localbkg_cases.npz: inputs and expected outputs of the
local background of the source catalogue (segmentation.SourceCatalog(...,
localbkg_width=L)).

photutils is not available.  What pins the rule is the catalogue photutils
itself wrote for the frame tests/golden/SUBDIV_ORIGIMG.fits: the reference's
results/SUBDIV_ORIGCAT.csv, kept unchanged as tests/golden/SUBDIV_ORIGCAT.csv
(103 rows, SourceCatalog(..., localbkg_width=5)).  This generator runs the
project's restatements on that frame -- make_golden_bkg.reference (box 60,
filter 3), tests/seg_ref.py, tests/deblend_ref.py (n_pixels=5) and
tests/localbkg_ref.py -- and stores the two filtered meshes (the tests rebuild
the maps with tests/bkg_ref.zoom), the deblended labels, the local backgrounds
and counts, the matching of rows against the CSV and the measured agreement.
It also stores small synthetic cases.  Run from the repository root with the
interpreter that has astropy 4.3.1 and scipy (python 3.9, as
make_golden_bkg.py):

    PYTHONDONTWRITEBYTECODE=1 python3.9 tests/golden/make_golden_localbkg.py

Asserted for every label of every case: the clipping of tests/localbkg_ref.py
leaves what ``astropy.stats.SigmaClip(3, maxiters=10)`` leaves; no value lies
within MARGIN (relative) of a clipping bound; | |mean - median| / std - 0.3 |
> BRANCH, so that a difference in the last bits of a sum cannot change which
pixels survive or which branch of L5 is taken.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import numpy as np  # noqa: E402

import make_golden_bkg as gb  # noqa: E402  (also patches numpy for astropy 4.3.1)
import bkg_ref  # noqa: E402
import deblend_ref  # noqa: E402
import localbkg_ref as ref  # noqa: E402
import seg_ref  # noqa: E402
from astropy.io import fits  # noqa: E402
from astropy.stats import SigmaClip  # noqa: E402

MARGIN, BRANCH = 1e-9, 1e-6


def boxes_of(labels):
    cat = seg_ref.catalog(np.ones(labels.shape), labels)
    box = np.stack([cat["bbox_xmin"], cat["bbox_xmax"], cat["bbox_ymin"], cat["bbox_ymax"]], 1)
    return box, cat["area"]


def run(data, labels, width, **kw):
    """local_background of every label, checked against astropy and the margins."""
    box, area = boxes_of(labels)
    res = ref.local_background(data, labels, box, area, width, **kw)
    for l in range(len(area)):
        if res["nsurv"][l] == 0:
            continue
        v = ref.values(data, labels, box[l], width)
        a = SigmaClip(sigma=kw.get("sigma", 3.0), maxiters=kw.get("maxiters", 10), cenfunc="median",
                      stdfunc="std")(v, masked=False)
        a = a[np.isfinite(a)]
        assert len(a) == res["nsurv"][l], (l, len(a), res["nsurv"][l])
    if res["margin"].min() < MARGIN:
        raise gb.MarginError(f"a value lies within {res['margin'].min():.2e} of a clipping bound")
    if res["branch"].min() < BRANCH:
        raise gb.MarginError(f"|mean - median| / std within {res['branch'].min():.2e} of 0.3")
    return res


def published(z):
    img = fits.getdata(os.path.join(HERE, "SUBDIV_ORIGIMG.fits"))  # (375, 375) >f4
    pub = ref.read_published(os.path.join(HERE, "SUBDIV_ORIGCAT.csv"))
    bk = gb.reference(img, (60, 60), (3, 3))
    bkg = bkg_ref.zoom(bk["bkg_mesh"], (60, 60), img.shape)
    rms = bkg_ref.zoom(bk["rms_mesh"], (60, 60), img.shape)
    assert np.max(np.abs(bkg - bk["bkg"])) < 1e-9 * np.max(np.abs(bkg))
    lab, n, sub, conv, _ = seg_ref.source_info(img, bkg, rms, 5)
    out, parent, st = deblend_ref.deblend(conv, lab, 5)  # raises on a tie within deblend_ref.MARGIN
    cat = seg_ref.catalog(sub, out, conv)
    box = np.stack([cat["bbox_xmin"], cat["bbox_xmax"], cat["bbox_ymin"], cat["bbox_ymax"]], 1)
    res = run(sub, out, 5.0)
    assert res["status"] == 0
    cor = ref.corrected(cat, res["lb"])
    match = ref.match_rows(cat, pub)
    ok = match >= 0
    m = match[ok]
    raw_gap = np.abs(cat["min_value"][m] - (pub["min_value"][ok] + pub["local_background"][ok]))
    lb_gap = np.abs(res["lb"][m] - pub["local_background"][ok])
    rel = np.abs(cor["segment_flux"][m] - pub["segment_flux"][ok]) / np.abs(pub["segment_flux"][ok])
    rel0 = np.abs(cat["segment_flux"][m] - pub["segment_flux"][ok]) / np.abs(pub["segment_flux"][ok])
    psum = pub["segment_flux"].sum()
    measured = np.array([len(cat["area"]), len(pub["area"]), ok.sum(), cat["segment_flux"].sum(),
                         cor["segment_flux"].sum(), psum, np.median(rel0), rel0.max(), np.median(rel),
                         rel.max(), np.median(lb_gap), lb_gap.max(), raw_gap.max()])
    names = ("segments, published rows, matched rows, sum flux uncorrected, sum flux corrected, "
             "published sum, rel flux diff uncorrected median, max, corrected median, max, "
             "|lb - published| median, max, max |raw min - (published min + lb)|")
    for nm, v in zip(names.split(", "), measured):
        print(f"  {nm}: {v!r}")
    print(f"  nlabels before deblending {n}, split {st['nsplit']} into {st['nchildren']}; "
          f"clip margin {res['margin'].min():.2e}, branch margin {res['branch'].min():.2e}")
    assert ok.sum() >= 97 and lb_gap.max() <= 2 * raw_gap.max()
    assert abs(cor["segment_flux"].sum() - psum) / psum <= 5e-4
    assert out.max() < 2 ** 15
    z["pub_bkg_mesh"], z["pub_rms_mesh"] = bk["bkg_mesh"], bk["rms_mesh"]
    z["pub_labels"] = out.astype(np.int16)
    z["pub_lb"], z["pub_ngather"], z["pub_nsurv"] = res["lb"], res["ngather"], res["nsurv"]
    z["pub_match"] = match.astype(np.int32)
    z["pub_measured"], z["pub_measured_names"] = measured, np.array(names)


def rect(labels, l, x0, x1, y0, y1):
    labels[y0:y1 + 1, x0:x1 + 1] = l


def synthetic(z):
    """Small cases; each stores data, labels (int16), width and the expected lb,
    ngather, nsurv, iters and status."""
    tags = []

    def put(tag, make, check=lambda r: True):
        def ok(c):
            r = run(*c)
            return check(r)
        seed, c = gb.first_seed(make, ok)
        data, labels, width = c
        r = run(data, labels, width)
        z[f"{tag}_data"], z[f"{tag}_labels"] = data, labels.astype(np.int16)
        z[f"{tag}_width"] = np.float64(width)
        for k in ("lb", "ngather", "nsurv", "iters"):
            z[f"{tag}_{k}"] = r[k]
        z[f"{tag}_status"] = np.int32(r["status"])
        tags.append(tag)
        print(f"  {tag}: seed {seed}, shape {data.shape}, labels {int(labels.max())}, width {width}, "
              f"ngather {r['ngather'].tolist()}, nsurv {r['nsurv'].tolist()}, iters "
              f"{r['iters'].tolist()}, status {r['status']}, margins {r['margin'].min():.1e} "
              f"{r['branch'].min():.1e}")

    def noise(rng, shape, level=10.0, sd=1.0):
        return level + sd * rng.standard_normal(shape)

    # box widths 1, 2, 3 and 6 with other heights: widths 2 and 6 put both
    # annulus edges on pixel centres (0.75 w and 0.75 w + L whole with cx on a
    # half pixel), width 1 a half-integer edge
    def widths(rng):
        d, lab = noise(rng, (33, 33)), np.zeros((33, 33), np.int32)
        rect(lab, 1, 6, 6, 5, 7)        # 1 x 3
        rect(lab, 2, 23, 24, 7, 7)      # 2 x 1
        rect(lab, 3, 5, 7, 21, 24)      # 3 x 4
        rect(lab, 4, 20, 25, 23, 24)    # 6 x 2
        d[lab > 0] += 50.0
        return d, lab, 2.0
    put("widths", widths, lambda r: r["ratio"].max() < 0.3)

    # half-integer width: the outer edges of widths 2 and 6 move off the centres
    def widths_half(rng):
        d, lab, _ = widths(rng)
        return d, lab, 2.5
    put("widths_half", widths_half)

    # an annulus cut by a corner, and annuli cut by two different borders
    def borders(rng):
        d, lab = noise(rng, (25, 29)), np.zeros((25, 29), np.int32)
        rect(lab, 1, 0, 2, 0, 1)
        rect(lab, 2, 26, 28, 10, 13)
        rect(lab, 3, 12, 15, 23, 24)
        return d, lab, 3.0
    put("borders", borders)

    # a second segment crosses the annulus of the first: its pixels are left out
    def crossed(rng):
        d, lab = noise(rng, (21, 27)), np.zeros((21, 27), np.int32)
        rect(lab, 1, 8, 11, 8, 11)
        rect(lab, 2, 13, 20, 9, 10)
        d[lab == 2] += 500.0
        return d, lab, 3.0
    put("crossed", crossed, lambda r: r["ngather"][0] == 12 * 12 - 6 * 6 - 6)

    # hemmed in: label 2 covers the annulus of label 1 but for 9 pixels
    def few(rng):
        d, lab = noise(rng, (21, 21)), np.full((21, 21), 2, np.int32)
        rect(lab, 1, 9, 11, 9, 11)
        lab[6, 6:15] = 0
        return d, lab, 2.0
    put("few", few, lambda r: r["ngather"][0] == 9 and r["status"] == ref.FEW)

    # one bright unlabelled pixel in the annulus, clipped in iteration 1
    def bright(rng):
        d, lab = noise(rng, (23, 23)), np.zeros((23, 23), np.int32)
        rect(lab, 1, 10, 12, 10, 12)
        d[7, 8] = 1000.0
        return d, lab, 3.0
    put("bright", bright, lambda r: r["ngather"][0] - r["nsurv"][0] == 1 and r["iters"][0] == 2)

    # outliers on three scales: at least three iterations remove values
    def cascade(rng):
        d, lab = noise(rng, (33, 33)), np.zeros((33, 33), np.int32)
        rect(lab, 1, 14, 18, 14, 18)
        ann = np.argwhere(ref.annulus(d.shape, (14, 18, 14, 18), 6.0))
        pick = ann[rng.permutation(len(ann))[:12]]
        for (y, x), v in zip(pick, [5000.0] * 3 + [300.0] * 4 + [40.0] * 5):
            d[y, x] = v
        return d, lab, 6.0
    put("cascade", cascade, lambda r: r["iters"][0] >= 4)

    # the three branches of L5: a constant annulus (std 0: the mean), a
    # symmetric one (2.5 median - 1.5 mean) and a skewed one (the median)
    def constant(rng):
        d, lab = np.full((21, 21), 3.0), np.zeros((21, 21), np.int32)
        rect(lab, 1, 9, 12, 9, 11)
        d[lab > 0] = 80.0
        return d, lab, 3.0
    put("constant", constant)

    def skewed(rng):
        d, lab = noise(rng, (27, 27), sd=0.05), np.zeros((27, 27), np.int32)
        rect(lab, 1, 11, 15, 11, 15)
        d[rng.random(d.shape) < 0.3] += 1.0
        return d, lab, 4.0

    def is_skewed(r):
        return r["ratio"][0] >= 0.3
    put("skewed", skewed, is_skewed)

    # NaN and infinite pixels in the annulus are skipped; float32 data
    def nonfinite(rng):
        d, lab = noise(rng, (23, 25)), np.zeros((23, 25), np.int32)
        rect(lab, 1, 10, 13, 9, 12)
        d[5, 6], d[6, 17], d[16, 8], d[16, 16] = np.nan, np.inf, -np.inf, np.nan
        return d, lab, 3.0
    put("nonfinite", nonfinite, lambda r: r["ngather"][0] == 12 * 12 - 6 * 6 - 4)

    def f32(rng):
        d, lab, w = widths(rng)
        return (d * 37.0).astype(np.float32), lab, w
    put("f32", f32)

    # the batch: three images of one shape with 4, 0 and 1 labels
    def one(rng):
        d, lab = noise(rng, (33, 33)), np.zeros((33, 33), np.int32)
        rect(lab, 1, 3, 9, 20, 22)
        return d, lab, 2.0
    put("one", one)
    z["tags"] = np.array(tags)


def main():
    z = {}
    print("published frame:")
    published(z)
    print("synthetic cases:")
    synthetic(z)
    path = os.path.join(HERE, "localbkg_cases.npz")
    np.savez_compressed(path, **z)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
