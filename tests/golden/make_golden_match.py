"""Generate tests/golden/match_cases.npz: inputs and expected outputs of the
catalogue cross-match (segmentation.match_catalogs).

What pins the rule is the reference's own output: its four published
cross-matched tables results/{SUBDIV,CROWDED_SUBDIV}_RESTORED{,_BETA}_MATCHED.csv,
made from the restored catalogue (table 1) and the original catalogue (table
2) of each frame by an external table tool.  This generator keeps, per
catalogue, the columns label, xcentroid, ycentroid, segment_flux, fwhm and
ellipticity, and per matched table label_1, label_2, Separation and the _1 /
_2 versions of those columns: data only.  Run from the repository root with the
directory that holds the reference's results:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_match.py <reference>/results

Asserted here: the restatement tests/match_ref.py reproduces every published
table at max_sep = 1.1 (pairs, order, Separation), the sorted walk equals the
rounds, and at 1.0 and 1.2 the pair sets differ from the published ones.

It also stores the small synthetic cases of tests/test_gpu_match.py with what
the restatement gives for them (match1, match2, sep1, npairs, status, rounds).
The uniform random catalogues of thousands of rows are not stored: the tests
draw them from a seeded generator.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import numpy as np  # noqa: E402

import match_ref as ref  # noqa: E402

# tag -> (restored catalogue, original catalogue, matched table)
PUBLISHED = {
    "subdiv": ("SUBDIV_RESTORED.csv", "SUBDIV_ORIGCAT.csv", "SUBDIV_RESTORED_MATCHED.csv"),
    "subdiv_beta": ("SUBDIV_RESTORED_BETA.csv", "SUBDIV_ORIGCAT.csv",
                    "SUBDIV_RESTORED_BETA_MATCHED.csv"),
    "crowded": ("CROWDED_SUBDIV_RESTORED.csv", "CROWDED_SUBDIV_ORIGCAT.csv",
                "CROWDED_SUBDIV_RESTORED_MATCHED.csv"),
    "crowded_beta": ("CROWDED_SUBDIV_RESTORED_BETA.csv", "CROWDED_SUBDIV_ORIGCAT.csv",
                     "CROWDED_SUBDIV_RESTORED_BETA_MATCHED.csv"),
}
MAX_SEP = 1.1


def published(z, results):
    for tag, (rest, orig, matched) in PUBLISHED.items():
        c1 = ref.read_csv(os.path.join(results, rest), ref.CAT_COLUMNS)
        c2 = ref.read_csv(os.path.join(results, orig), ref.CAT_COLUMNS)
        m1 = ref.read_csv(os.path.join(results, matched), ref.CAT_COLUMNS, "_1")
        m2 = ref.read_csv(os.path.join(results, matched), ref.CAT_COLUMNS, "_2")
        res = ref.match_greedy(c1["xcentroid"], c1["ycentroid"], c2["xcentroid"], c2["ycentroid"],
                               MAX_SEP)
        i, j, sep = ref.pairs_of(res)
        assert np.array_equal(c1["label"][i], m1["label"]), tag
        assert np.array_equal(c2["label"][j], m2["label"]), tag
        rel = np.max(np.abs(sep - m1["Separation"]) / m1["Separation"])
        for nm in ref.CAT_COLUMNS:  # the joined columns are the source rows, bit for bit
            assert np.array_equal(c1[nm][i], m1[nm]) and np.array_equal(c2[nm][j], m2[nm]), (tag, nm)
        rr = ref.match_rounds(c1["xcentroid"], c1["ycentroid"], c2["xcentroid"], c2["ycentroid"],
                              MAX_SEP)
        assert np.array_equal(rr["match1"], res["match1"])
        for other in (1.0, 1.2):
            o = ref.match_greedy(c1["xcentroid"], c1["ycentroid"], c2["xcentroid"],
                                 c2["ycentroid"], other)
            assert not np.array_equal(o["match1"], res["match1"]), (tag, other)
        print(f"  {tag}: {len(i)} pairs of {len(c1['label'])} x {len(c2['label'])}, Separation "
              f"within {rel:.2e} relative, largest {sep.max():.4f}, rounds {rr['rounds']}")
        for nm in ref.CAT_COLUMNS:
            z[f"{tag}_cat1_{nm}"], z[f"{tag}_cat2_{nm}"] = c1[nm], c2[nm]
            z[f"{tag}_pub_{nm}_1"], z[f"{tag}_pub_{nm}_2"] = m1[nm], m2[nm]
        z[f"{tag}_pub_Separation"] = m1["Separation"]
    z["published"] = np.array(list(PUBLISHED))


def synthetic(z):
    tags = []

    def put(tag, x1, y1, x2, y2, max_sep, **kw):
        x1, y1, x2, y2 = (np.array(v, dtype=np.float64) for v in (x1, y1, x2, y2))  # copies
        g = ref.match_greedy(x1, y1, x2, y2, max_sep, **kw)
        r = ref.match_rounds(x1, y1, x2, y2, max_sep, **kw)
        for k in ("match1", "match2", "npairs", "status"):
            assert np.array_equal(g[k], r[k]), (tag, k)
        assert np.array_equal(g["sep1"], r["sep1"], equal_nan=True), tag
        z[f"{tag}_x1"], z[f"{tag}_y1"], z[f"{tag}_x2"], z[f"{tag}_y2"] = x1, y1, x2, y2
        z[f"{tag}_max_sep"] = np.float64(max_sep)
        for k, v in kw.items():
            z[f"{tag}_{k}"] = np.array(v, dtype=np.int32)
        for k in ("match1", "match2", "sep1"):
            z[f"{tag}_{k}"] = r[k]
        for k in ("npairs", "status", "rounds"):
            z[f"{tag}_{k}"] = np.int32(r[k])
        tags.append(tag)
        print(f"  {tag}: {len(x1)} x {len(x2)}, max_sep {max_sep!r}, pairs {r['npairs']}, status "
              f"{r['status']}, rounds {r['rounds']} {r['accepted'][:6]}")
        return r

    e = np.zeros(0)
    put("empty1", e, e, [1.0, 2.0], [1.0, 2.0], 1.1)
    put("empty2", [1.0, 2.0], [1.0, 2.0], e, e, 1.1)
    put("empty_both", e, e, e, e, 1.1)
    put("one_inside", [10.0], [10.0], [10.5], [10.5], 1.1)
    put("one_outside", [10.0], [10.0], [11.0], [11.0], 1.1)
    r = put("bound_in", [0.0], [0.0], [0.0], [1.5], 1.5)  # the bound is inclusive
    assert r["npairs"] == 1 and r["sep1"][0] == 1.5
    r = put("bound_out", [0.0], [0.0], [0.0], [1.5], np.nextafter(1.5, 0.0))
    assert r["npairs"] == 0
    # a 3 x 3 lattice against itself shifted by half a cell: four equal distances
    # per inner point, broken by the indices
    gy, gx = np.mgrid[0:3, 0:3].astype(np.float64)
    r = put("lattice", gx.ravel(), gy.ravel(), gx.ravel() + 0.5, gy.ravel() + 0.5, 1.0)
    assert r["npairs"] == 9 and len(np.unique(r["sep1"])) == 1
    # duplicated points in both catalogues
    put("duplicates", [5.0, 5.0, 5.0, 9.0], [5.0, 5.0, 5.0, 9.0], [5.0, 5.0, 9.0, 9.0, 9.0],
        [5.0, 5.0, 9.0, 9.0, 9.0], 0.5)
    # the chain: the orphan-rescan logic's case
    r = put("chain", *ref.chain(40), 2.0)
    assert r["rounds"] == 40 and r["accepted"] == [1] * 40 and r["npairs"] == 40
    # valid masks and non-finite coordinates (a masked row may hold anything)
    rng = np.random.default_rng(7)
    x1, y1 = rng.uniform(0, 30, 40), rng.uniform(0, 30, 40)
    x2, y2 = x1[::-1] + rng.normal(0, 0.4, 40), y1[::-1] + rng.normal(0, 0.4, 40)
    v1, v2 = np.ones(40, np.int32), np.ones(40, np.int32)
    v1[[3, 17]], v2[[0, 8, 30]] = 0, (0, -1, 0)
    x1[3], y1[5], x2[8], x2[12], y2[20] = np.nan, np.inf, np.nan, -np.inf, np.nan
    r = put("masked", x1, y1, x2, y2, 1.1, valid1=v1, valid2=v2)
    assert r["status"] == ref.NONFINITE and (r["match1"][[3, 5, 17]] == -1).all()
    y1[5], x2[12], y2[20] = 1.0, 2.0, 3.0
    r = put("masked_finite", x1, y1, x2, y2, 1.1, valid1=v1, valid2=v2)  # the rest hides behind valid
    assert r["status"] == 0
    # more rows announced than the arrays hold
    x1, x2 = np.nan_to_num(x1, nan=15.0), np.nan_to_num(x2, nan=15.0)
    r = put("over_cap", x1[:20], y1[:20], x2[20:], y2[20:], 1.1, n1=25, n2=20)
    assert r["status"] == ref.OVER_CAP
    put("short_n", x1, y1, x2, y2, 1.1, n1=11, n2=33)
    # the batch: six images with 0 .. 300 rows
    for k, (n1, n2) in enumerate(((0, 17), (1, 1), (64, 65), (129, 300), (300, 128), (255, 0))):
        a, b = rng.uniform(0, 60, n1), rng.uniform(0, 60, n1)
        m = min(n1, n2)
        c = np.concatenate([a[:m] + rng.normal(0, 0.5, m), rng.uniform(0, 60, n2 - m)])
        d = np.concatenate([b[:m] + rng.normal(0, 0.5, m), rng.uniform(0, 60, n2 - m)])
        p = rng.permutation(n2)
        put(f"batch{k}", a, b, c[p], d[p], 1.5)
    z["tags"] = np.array(tags)


def main():
    results = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BSGP_REFERENCE_RESULTS")
    if not results:
        sys.exit(__doc__)
    z = {}
    print("published tables:")
    published(z, results)
    print("synthetic cases:")
    synthetic(z)
    path = os.path.join(HERE, "match_cases.npz")
    np.savez_compressed(path, **z)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
