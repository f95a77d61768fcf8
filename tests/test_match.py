"""Host-side checks of the catalogue cross-match (no device): the restatement
tests/match_ref.py against the reference's four published cross-matched tables
(tests/golden/match_cases.npz, made by tests/golden/make_golden_match.py), the
sorted walk against the rounds, the fixture reproducing itself, the host
functions matched_columns / matched_metrics / check_match_args, and the entry
point in the header, the binding and the built library."""
import inspect
import os
import re

import numpy as np
import pytest

import match_ref as ref
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLISHED = {"subdiv": (62, 134, 103), "subdiv_beta": (62, 126, 103), "crowded": (121, 321, 392),
             "crowded_beta": (35, 407, 392)}
RADII = (1.1, 2.0, 3.0, 5.0, 10.0, 40.0)


@pytest.fixture(scope="module")
def sg():
    import segmentation
    return segmentation


@pytest.fixture(scope="module")
def fx():
    return golden("match_cases.npz")


def cats(fx, tag):
    """(restored, original) catalogue of a published table, as dicts."""
    return tuple({nm: fx[f"{tag}_cat{k}_{nm}"] for nm in ref.CAT_COLUMNS} for k in (1, 2))


def as_match(sg, res, c1=None, c2=None):
    """A restatement's result as the CatalogMatch match_catalogs would return."""
    return sg.CatalogMatch([res["match1"]], [res["match2"]], [res["sep1"]], [res["status"]],
                           [None if c1 is None else c1["label"]],
                           [None if c2 is None else c2["label"]])


def synthetic_case(fx, tag):
    kw = {k: fx[f"{tag}_{k}"] for k in ("valid1", "valid2") if f"{tag}_{k}" in fx}
    kw.update({k: int(fx[f"{tag}_{k}"]) for k in ("n1", "n2") if f"{tag}_{k}" in fx})
    return [fx[f"{tag}_{k}"] for k in ("x1", "y1", "x2", "y2")] + [float(fx[f"{tag}_max_sep"])], kw


@pytest.mark.parametrize("tag", sorted(PUBLISHED))
def test_restatement_reproduces_the_published_table(sg, fx, tag):
    c1, c2 = cats(fx, tag)
    npairs, n1, n2 = PUBLISHED[tag]
    assert (len(c1["label"]), len(c2["label"])) == (n1, n2)
    res = ref.match_greedy(c1["xcentroid"], c1["ycentroid"], c2["xcentroid"], c2["ycentroid"], 1.1)
    m = as_match(sg, res, c1, c2)
    assert m.n_pairs == npairs == res["npairs"] and m.status == 0
    # the pair set, in the published order (by the restored row)
    assert np.array_equal(m.labels1, fx[f"{tag}_pub_label_1"])
    assert np.array_equal(m.labels2, fx[f"{tag}_pub_label_2"])
    assert np.all(np.diff(m.idx1) > 0)
    # Separation: the bar is 1e-11 relative; measured with this numpy: 0 (every value bit-equal)
    pub = fx[f"{tag}_pub_Separation"]
    rel = np.max(np.abs(m.separation - pub) / pub)
    print(f"{tag}: Separation within {rel:.2e} relative of the published column")
    assert rel <= 1e-11
    assert m.separation.max() <= 1.1
    # the joined columns, bit for bit
    joined = sg.matched_columns(m, c1, c2)
    assert list(joined) == [f"{nm}_1" for nm in ref.CAT_COLUMNS] + \
        [f"{nm}_2" for nm in ref.CAT_COLUMNS] + ["Separation"]
    for nm in ref.CAT_COLUMNS:
        for k in ("_1", "_2"):
            assert np.array_equal(joined[nm + k], fx[f"{tag}_pub_{nm}{k}"]), nm + k
    assert len(m.unmatched1) == n1 - npairs and len(m.unmatched2) == n2 - npairs
    only = sg.matched_columns(m, c1, c2, columns=("fwhm",))
    assert list(only) == ["fwhm_1", "fwhm_2", "Separation"]


@pytest.mark.parametrize("tag", sorted(PUBLISHED))
def test_other_radii_give_other_tables(fx, tag):
    """What pins 1.1: the largest published separation is 1.0932 and the
    smallest unpublished one 1.1008."""
    c1, c2 = cats(fx, tag)
    xy = (c1["xcentroid"], c1["ycentroid"], c2["xcentroid"], c2["ycentroid"])
    at = {r: ref.match_greedy(*xy, r)["match1"] for r in (1.0, 1.1, 1.2)}
    assert not np.array_equal(at[1.0], at[1.1]) and not np.array_equal(at[1.2], at[1.1])


@pytest.mark.parametrize("tag", sorted(PUBLISHED))
def test_greedy_equals_rounds_on_the_published_catalogues(fx, tag):
    c1, c2 = cats(fx, tag)
    xy = (c1["xcentroid"], c1["ycentroid"], c2["xcentroid"], c2["ycentroid"])
    most = 0
    for r in RADII:
        g, q = ref.match_greedy(*xy, r), ref.match_rounds(*xy, r)
        for k in ("match1", "match2", "npairs", "status"):
            assert np.array_equal(g[k], q[k]), (r, k)
        assert np.array_equal(g["sep1"], q["sep1"], equal_nan=True)
        assert 1 <= q["rounds"] <= min(len(xy[0]), len(xy[2])) and sum(q["accepted"]) == q["npairs"]
        most = max(most, q["rounds"])
    assert most >= 2  # the wider radii hold real conflicts


def test_fixture_reproduces_itself_and_greedy_equals_rounds(fx):
    assert len(fx["tags"]) == 20
    for tag in fx["tags"]:
        args, kw = synthetic_case(fx, tag)
        g, q = ref.match_greedy(*args, **kw), ref.match_rounds(*args, **kw)
        for res in (g, q):
            for k in ("match1", "match2", "npairs", "status"):
                assert np.array_equal(res[k], fx[f"{tag}_{k}"]), (tag, k)
            assert np.array_equal(res["sep1"], fx[f"{tag}_sep1"], equal_nan=True), tag
        assert q["rounds"] == int(fx[f"{tag}_rounds"])


def test_fixture_cases_are_what_they_are_for(fx):
    assert fx["bound_in_npairs"] == 1 and fx["bound_in_sep1"][0] == 1.5 == fx["bound_in_max_sep"]
    assert fx["bound_out_npairs"] == 0 and fx["bound_out_max_sep"] == np.nextafter(1.5, 0.0)
    # the lattice: nine equal separations; the indices break the ties
    assert fx["lattice_npairs"] == 9 and len(np.unique(fx["lattice_sep1"])) == 1
    assert fx["lattice_match1"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8] and fx["lattice_rounds"] == 5
    assert fx["duplicates_match1"].tolist() == [0, 1, -1, 2]
    # the chain: 40 accepting rounds of one pair each, from the far end
    x1, y1, x2, y2 = ref.chain(40)
    assert np.array_equal(x1, fx["chain_x1"]) and np.array_equal(x2, fx["chain_x2"])
    q = ref.match_rounds(x1, y1, x2, y2, 2.0)
    assert q["rounds"] == 40 and q["accepted"] == [1] * 40
    assert q["match1"].tolist() == list(range(40))
    assert fx["masked_status"] == ref.NONFINITE and fx["masked_finite_status"] == 0
    assert (fx["masked_match1"][[3, 5, 17]] == -1).all() and np.isnan(fx["masked_sep1"][[3, 5, 17]]).all()
    assert (fx["masked_match2"][[0, 8, 12, 20, 30]] == -1).all()
    assert fx["over_cap_status"] == ref.OVER_CAP and fx["over_cap_n1"] == 25 > len(fx["over_cap_x1"])
    assert (fx["short_n_match1"][11:] == -1).all() and (fx["short_n_match2"][33:] == -1).all()
    assert [len(fx[f"batch{k}_x1"]) for k in range(6)] == [0, 1, 64, 129, 300, 255]


@pytest.mark.parametrize("tag", sorted(PUBLISHED))
def test_matched_metrics_on_the_published_pairs(sg, fx, tag):
    rest, orig = cats(fx, tag)
    res = ref.match_greedy(rest["xcentroid"], rest["ycentroid"], orig["xcentroid"],
                           orig["ycentroid"], 1.1)
    got = sg.matched_metrics(orig, rest, match=as_match(sg, res, rest, orig))
    p = {k: fx[f"{tag}_pub_{k}"] for k in ("segment_flux_1", "segment_flux_2", "fwhm_1", "fwhm_2",
                                            "ellipticity_1", "ellipticity_2", "label_1", "label_2")}
    want = dict(flux_fractional_difference=1 - p["segment_flux_1"] / p["segment_flux_2"],
                fwhm_ratio=p["fwhm_1"] / p["fwhm_2"],
                ellipticity_ratio=p["ellipticity_1"] / p["ellipticity_2"])
    for k, v in want.items():
        assert np.array_equal(got[k], v), k
        assert got["median_" + k] == np.median(v)
    assert np.array_equal(got["restored_label"], p["label_1"])
    assert np.array_equal(got["orig_label"], p["label_2"])
    assert np.array_equal(got["separation"], res["sep1"][res["match1"] >= 0])
    npairs, n1, n2 = PUBLISHED[tag]
    assert (got["n_pairs"], got["n_restored"], got["n_orig"]) == (npairs, n1, n2)


def test_matched_metrics_without_a_pair(sg):
    a = dict(xcentroid=np.array([1.0]), ycentroid=np.array([1.0]), segment_flux=np.array([2.0]),
             fwhm=np.array([3.0]), ellipticity=np.array([0.1]))
    b = dict(a, xcentroid=np.array([9.0]))
    res = ref.match_greedy(b["xcentroid"], b["ycentroid"], a["xcentroid"], a["ycentroid"], 1.1)
    got = sg.matched_metrics(a, b, match=as_match(sg, res))
    assert got["n_pairs"] == 0 and len(got["fwhm_ratio"]) == 0 and np.isnan(got["median_fwhm_ratio"])
    assert got["orig_label"] is None and got["restored_label"] is None


def test_check_match_args(sg):
    assert sg.check_match_args(1.1) == (1.1, 0) and sg.check_match_args(np.int64(2), "auto") == (2.0, 0)
    assert sg.check_match_args(0, "lds", 3, 3, 4000, 96) == (0.0, 1)
    assert sg.check_match_args(1.1, "global", 1, 1, 16384, 16384) == (1.1, 2)
    for bad in (-0.1, float("nan"), float("inf"), "1.1", None, True):
        with pytest.raises(ValueError, match="max_sep"):
            sg.check_match_args(bad)
    for bad in ("LDS", 1, "fast", b"lds"):
        with pytest.raises(ValueError, match="path"):
            sg.check_match_args(1.1, bad)
    with pytest.raises(ValueError, match="batch"):
        sg.check_match_args(1.1, None, 2, 3)
    with pytest.raises(ValueError, match="16384"):
        sg.check_match_args(1.1, None, 1, 1, 16385, 1)
    with pytest.raises(ValueError, match="4096"):
        sg.check_match_args(1.1, "lds", 1, 1, 4000, 97)
    # the checks come before the device is asked for
    with pytest.raises(ValueError, match="batch"):
        sg.match_catalogs([([1.0], [1.0])], [([1.0], [1.0])] * 2)
    with pytest.raises(ValueError, match="batch"):
        sg.match_catalogs([([1.0], [1.0])], ([1.0], [1.0]))
    with pytest.raises(ValueError, match="max_sep"):
        sg.match_catalogs(([1.0], [1.0]), ([1.0], [1.0]), max_sep=-1)
    p = inspect.signature(sg.match_catalogs).parameters
    assert tuple(p) == ("cat1", "cat2", "max_sep", "device_out", "path")
    assert (p["max_sep"].default, p["device_out"].default, p["path"].default) == (1.1, False, None)
    assert inspect.signature(sg.matched_metrics).parameters["max_sep"].default == 1.1
    assert (sg.MATCH_LDS_MAX, sg.MATCH_MAX) == (4096, 16384)


def test_there_is_no_cpu_fallback(sg, monkeypatch):
    import _bsgp

    def no_gpu():
        raise RuntimeError("no GPU here")
    monkeypatch.setattr(_bsgp, "require_gpu", no_gpu)
    with pytest.raises(RuntimeError, match="no GPU here"):
        sg.match_catalogs(([1.0], [1.0]), ([1.0], [1.0]))


def test_symbol_in_header_binding_and_library():
    import _bsgp
    with open(os.path.join(ROOT, "include", "bsgp.h")) as f:
        head = f.read()
    m = re.search(r"int bsgp_match_catalogs\(([^;]*)\);", head)
    assert m, "bsgp_match_catalogs is not declared in include/bsgp.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert "bsgp_match_catalogs" in _bsgp.EXPORTED
    fn = _bsgp.lib().bsgp_match_catalogs  # AttributeError if the built library lacks it
    assert len(fn.argtypes) == len(args) == 23
    for name, val in (("BSGP_MATCH_LDS_MAX", 4096), ("BSGP_MATCH_MAX", 16384), ("BSGP_MATCH_AUTO", 0),
                      ("BSGP_MATCH_LDS", 1), ("BSGP_MATCH_GLOBAL", 2), ("BSGP_MATCH_NONFINITE", 1),
                      ("BSGP_MATCH_OVER_CAP", 2)):
        assert re.search(rf"#define {name} {val}\b", head) and getattr(_bsgp, name) == val
    assert (ref.NONFINITE, ref.OVER_CAP) == (_bsgp.BSGP_MATCH_NONFINITE, _bsgp.BSGP_MATCH_OVER_CAP)
    for rule in ("M1", "M2", "M3", "M4", "M5", "M6"):
        assert re.search(rf"\b{rule}\b", head), rule


def test_c_abi_argument_checks():
    """Every error return of the entry point comes before the device is
    touched (tests/test_gpu_match.py repeats them where there is one)."""
    import _bsgp
    ref.check_abi_errors(_bsgp)
