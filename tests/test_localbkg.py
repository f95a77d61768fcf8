"""Host-side checks of the local background of the source catalogue (no
device): the restatement tests/localbkg_ref.py against the catalogue photutils
itself wrote for tests/golden/SUBDIV_ORIGIMG.fits (tests/golden/SUBDIV_ORIGCAT.csv,
``SourceCatalog(..., localbkg_width=5)``), the fixture
tests/golden/localbkg_cases.npz reproducing itself, the entry point in the
header, the ctypes binding and the built library, and the argument checks of
both layers."""
import inspect
import os
import re

import numpy as np
import pytest

import localbkg_ref as ref
from conftest import GOLDEN, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sg():
    import segmentation
    return segmentation


@pytest.fixture(scope="module")
def fx():
    return golden("localbkg_cases.npz")


@pytest.fixture(scope="module")
def pub():
    p = ref.read_published(os.path.join(GOLDEN, "SUBDIV_ORIGCAT.csv"))
    assert len(p["area"]) == 103
    return p


@pytest.fixture(scope="module")
def frame(fx):
    import fits_io
    _, img = fits_io.read_fits(os.path.join(GOLDEN, "SUBDIV_ORIGIMG.fits"))
    assert img.shape == (375, 375) and img.dtype == np.float32
    sub, labels, cat, box = ref.published_frame(fx, img)
    res = ref.local_background(sub, labels, box, cat["area"], 5.0)
    return sub, labels, cat, box, res


def test_restatement_against_the_published_catalogue(fx, pub, frame):
    sub, labels, cat, box, res = frame
    assert res["status"] == 0 and len(cat["area"]) == 104
    assert np.array_equal(res["lb"], fx["pub_lb"])  # the fixture reproduces itself
    assert np.array_equal(res["ngather"], fx["pub_ngather"])
    assert np.array_equal(res["nsurv"], fx["pub_nsurv"])
    assert np.array_equal(ref.match_rows(cat, pub), fx["pub_match"])
    cor = ref.corrected(cat, res["lb"])
    got = ref.check_against_published(cat, res["lb"], cor["segment_flux"], cat["min_value"], pub)
    assert got["matched"] == 97
    # what the correction is worth: without it the sum is 2.8 % too high
    psum = pub["segment_flux"].sum()
    assert abs(cat["segment_flux"].sum() - psum) / psum > 2e-2
    # the margins that keep a last-bit difference of a sum from changing a survivor or a branch
    assert res["margin"].min() > 1e-9 and res["branch"].min() > 1e-6


def test_the_other_conventions_miss_the_published_catalogue(pub, frame):
    """What pins the rule: non-strict comparisons, leaving out only the
    source's own pixels, or a plain clipped median all miss the published
    local backgrounds by ten times the background-map disagreement."""
    sub, labels, cat, box, res = frame
    match = ref.match_rows(cat, pub)
    ok = match >= 0
    m = match[ok]
    want = pub["local_background"][ok]

    def gap(lb):
        return np.abs(lb[m] - want).max()

    assert gap(res["lb"]) < 0.13
    median = np.zeros(len(box))
    own = np.zeros(len(box))
    for l in range(len(box)):
        s = ref.values(sub, labels, box[l], 5.0)
        lo, hi, _, med, _, _, _ = ref.clip_sorted(s)
        median[l] = med
        s = ref.values(sub, np.where(labels == l + 1, labels, 0), box[l], 5.0)
        lo, hi, _, med, mean, sd, _ = ref.clip_sorted(s)
        own[l] = ref.mode_estimate(mean, med, sd)
    assert gap(median) > 1.0 and gap(own) > 1.0, (gap(median), gap(own))


@pytest.mark.parametrize("tag", ("widths", "widths_half", "borders", "crossed", "few", "bright",
                                 "cascade", "constant", "skewed", "nonfinite", "f32", "one"))
def test_fixture_reproduces_itself(fx, tag):
    import seg_ref
    assert tag in fx["tags"]
    d, lab, w = fx[f"{tag}_data"], fx[f"{tag}_labels"].astype(np.int32), float(fx[f"{tag}_width"])
    cat = seg_ref.catalog(np.ones(d.shape), lab)
    box = np.stack([cat["bbox_xmin"], cat["bbox_xmax"], cat["bbox_ymin"], cat["bbox_ymax"]], 1)
    res = ref.local_background(d, lab, box, cat["area"], w)
    for k in ("lb", "ngather", "nsurv", "iters"):
        assert np.array_equal(res[k], fx[f"{tag}_{k}"]), k
    assert res["status"] == int(fx[f"{tag}_status"])
    assert res["margin"].min() > 1e-9 and res["branch"].min() > 1e-6


def test_fixture_cases_are_what_they_are_for(fx):
    assert fx["few_status"] == ref.FEW and fx["few_lb"][0] == 0.0 and fx["few_ngather"][0] == 9
    assert fx["bright_ngather"][0] - fx["bright_nsurv"][0] == 1 and fx["bright_iters"][0] == 2
    assert fx["cascade_iters"][0] >= 4  # three iterations remove values, the last finds none
    assert fx["constant_lb"][0] == 3.0
    assert fx["crossed_ngather"][0] == 12 * 12 - 6 * 6 - 6
    assert fx["nonfinite_ngather"][0] == 12 * 12 - 6 * 6 - 4
    assert fx["f32_data"].dtype == np.float32
    # strict comparisons: box width 2 with L = 2 has both edges on pixel centres
    # (|x - cx| = 1.5 is outside the inner rectangle's exclusion, 3.5 outside the outer)
    a = ref.annulus((9, 12), (5, 6, 4, 4), 2.0)
    assert a[4].tolist() == [False, False, False, True, True, False, False, True, True, False,
                             False, False]


def test_symbol_in_header_binding_and_library():
    import _bsgp
    with open(os.path.join(ROOT, "include", "bsgp.h")) as f:
        head = f.read()
    m = re.search(r"int bsgp_segment_local_background\(([^;]*)\);", head)
    assert m, "bsgp_segment_local_background is not declared in include/bsgp.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert "bsgp_segment_local_background" in _bsgp.EXPORTED
    fn = _bsgp.lib().bsgp_segment_local_background  # AttributeError if the built library lacks it
    assert len(fn.argtypes) == len(args) == 19
    for name, val in (("BSGP_LOCALBKG_MAX", 8192), ("BSGP_LOCALBKG_FEW", 1),
                      ("BSGP_LOCALBKG_OVER_CAP", 2)):
        assert re.search(rf"#define {name} {val}\b", head) and getattr(_bsgp, name) == val
    assert _bsgp.lib().bsgp_abi_version() == 3
    for rule in ("L1", "L2", "L3", "L4", "L5", "L6"):
        assert re.search(rf"\b{rule}\b", head), rule


def test_c_abi_argument_checks():
    import _bsgp
    L = _bsgp.lib()
    p = 8  # a non-NULL pointer that is never followed: the checks come first

    def call(data=p, dtype=1, B=1, H=4, W=4, cap=1, width=5.0, sigma=3.0, maxiters=10, min_pixels=10,
             apply=1, fcols=p, lb=p):
        return L.bsgp_segment_local_background(data, dtype, p, B, H, W, cap, None, p, fcols, width,
                                               sigma, maxiters, min_pixels, apply, lb, p, p, None)

    for kw, word in ((dict(width=0.0), b"localbkg_width"), (dict(width=-1.0), b"localbkg_width"),
                     (dict(width=float("inf")), b"localbkg_width"),
                     (dict(width=float("nan")), b"localbkg_width"), (dict(sigma=0.0), b"sigma"),
                     (dict(sigma=float("nan")), b"sigma"), (dict(maxiters=-1), b"maxiters"),
                     (dict(min_pixels=0), b"min_pixels"), (dict(dtype=2), b"dtype"),
                     (dict(cap=0), b"cap"), (dict(data=None), b"data"), (dict(B=-1), b"B"),
                     (dict(H=0), b"H"), (dict(fcols=None), b"f64_cols"), (dict(lb=None), b"lb_out")):
        assert call(**kw) == _bsgp.BSGP_ERR_ARG and word in L.bsgp_last_error(), kw
    for kw in (dict(B=65536), dict(H=65536, W=65536)):
        assert call(**kw) == _bsgp.BSGP_ERR_UNSUPPORTED, kw
    # no image: a no-op that follows no pointer
    assert L.bsgp_segment_local_background(None, 1, None, 0, 4, 4, 1, None, None, None, 5.0, 3.0, 10,
                                           10, 1, None, None, None, None) == 0


def test_python_argument_checks_and_signatures(sg):
    import subdivisions
    d, lab = np.ones((6, 7)), np.ones((6, 7), np.int32)
    for bad in (-1, float("nan"), float("inf"), "5", None, True):
        with pytest.raises(ValueError, match="localbkg_width"):
            sg.SourceCatalog(d, lab, localbkg_width=bad)
        with pytest.raises(ValueError, match="localbkg_width"):
            sg.source_info(d, 3, localbkg_width=bad)
        with pytest.raises(ValueError, match="localbkg_width"):
            sg.catalog_flux_fraction_score(d, 3, localbkg_width=bad)
        with pytest.raises(ValueError, match="localbkg_width"):
            subdivisions._segment_flux({"flux": "segments"}, d[None], 3, localbkg_width=bad)
    assert sg.check_localbkg_width(0) == 0.0 and sg.check_localbkg_width(np.int64(5)) == 5.0
    last = {sg.SourceCatalog.__init__: ("localbkg_width",),
            sg.source_info: ("localbkg_width",),
            sg.segment_flux_sums: ("localbkg_width", "deblend", "large_parents"),
            sg.catalog_flux_fraction_score: ("localbkg_width", "deblend")}
    for fn, names in last.items():
        p = inspect.signature(fn).parameters
        assert tuple(p)[-len(names):] == names, fn
        for nm in names:
            assert p[nm].default in (0, False) and p[nm].default is not None, (fn, nm)
    assert tuple(inspect.signature(sg.SourceCatalog.__init__).parameters)[1:] == (
        "data", "segment_img", "convolved_data", "background", "device_out", "localbkg_width")
    for fn in (subdivisions.sgp_subdivisions, subdivisions.sgp_subdivisions_multistart):
        p = inspect.signature(fn).parameters
        assert p["flux_localbkg_width"].default == 0 and p["flux_deblend"].default is False
    assert sg.LOCALBKG_MAX == 8192 and issubclass(sg.LocalBackgroundCapWarning, UserWarning)
    assert (sg.LOCALBKG_SIGMA, sg.LOCALBKG_MAXITERS, sg.LOCALBKG_MIN_PIXELS) == (3.0, 10, 10)


def test_width_zero_keeps_the_keyerror_and_there_is_no_cpu_fallback(sg, monkeypatch):
    assert "localbkg_width" in sg.UNAVAILABLE["local_background"]
    assert "background" in sg.UNAVAILABLE["local_background"]
    cat = sg.SourceCatalog.__new__(sg.SourceCatalog)
    cat._cols, cat.batched = {"label": [np.arange(1, 3)]}, False
    with pytest.raises(KeyError, match="localbkg_width"):
        cat["local_background"]
    with pytest.raises(AttributeError, match="localbkg_width"):
        cat.local_background
    for nm in ("sky_centroid", "segment_fluxerr"):
        with pytest.raises(KeyError, match="not available"):
            cat[nm]
    cat._cols["local_background"] = [np.array([1.5, 2.5])]  # measured: found before UNAVAILABLE
    assert cat["local_background"].tolist() == [1.5, 2.5]
    assert list(cat.to_dict(("label", "local_background"))) == ["label", "local_background"]
    assert "local_background" not in sg.COLUMNS

    import _bsgp

    def no_gpu():
        raise RuntimeError("no GPU here")
    monkeypatch.setattr(_bsgp, "require_gpu", no_gpu)
    d, lab = np.ones((6, 7)), np.ones((6, 7), np.int32)
    with pytest.raises(RuntimeError, match="no GPU here"):
        sg.SourceCatalog(d, lab, localbkg_width=5)
