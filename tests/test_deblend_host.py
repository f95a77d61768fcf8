"""Host-side checks of the deblending (no device): the argument checks of
``deblend_sources`` / ``SourceFinder`` / ``source_info``, the D7 numbering
rule, the consistency of tests/golden/deblend_cases.npz with seg_cases.npz and
the restatement tests/deblend_ref.py on a small case."""
import inspect

import numpy as np
import pytest

import deblend_ref
from conftest import golden


@pytest.fixture(scope="module")
def sg():
    import segmentation
    return segmentation


@pytest.fixture(scope="module")
def fx():
    return golden("deblend_cases.npz")


@pytest.fixture(scope="module")
def seg():
    return golden("seg_cases.npz")


def test_argument_checks_raise_before_the_device(sg):
    d, lab = np.ones((6, 7)), np.ones((6, 7), np.int32)
    with pytest.raises(ValueError, match="sinh"):
        sg.deblend_sources(d, lab, 1, mode="sinh")
    with pytest.raises(ValueError, match="mode must be"):
        sg.deblend_sources(d, lab, 1, mode="log")
    with pytest.raises(ValueError, match="relabel=False"):
        sg.deblend_sources(d, lab, 1, relabel=False)
    with pytest.raises(ValueError, match="nlevels"):
        sg.deblend_sources(d, lab, 1, nlevels=0)
    for c in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="contrast"):
            sg.deblend_sources(d, lab, 1, contrast=c)
    with pytest.raises(ValueError, match="npixels"):
        sg.deblend_sources(d, lab, 0)
    with pytest.raises(ValueError, match="connectivity"):
        sg.deblend_sources(d, lab, 1, connectivity=6)
    with pytest.raises(ValueError, match="does not match"):
        sg.deblend_sources(d, lab[:, :6], 1)
    with pytest.raises(ValueError, match="does not match"):
        sg.deblend_sources(d[None], lab, 1)
    with pytest.raises(ValueError, match="sinh"):
        sg.SourceFinder(5, mode="sinh")
    with pytest.raises(ValueError, match="relabel=False"):
        sg.SourceFinder(5, relabel=False)
    with pytest.raises(ValueError, match="nlevels"):
        sg.source_info(d, 3, deblend=True, nlevels=0)


def test_signatures(sg):
    p = inspect.signature(sg.deblend_sources).parameters
    assert list(p)[:9] == ["data", "segment_img", "npixels", "labels", "nlevels", "contrast", "mode",
                           "connectivity", "relabel"]
    assert (p["nlevels"].default, p["contrast"].default, p["mode"].default,
            p["connectivity"].default, p["relabel"].default) == (32, 0.001, "exponential", 8, True)
    f = inspect.signature(sg.SourceFinder.__init__).parameters
    assert f["deblend"].default is True and "progress_bar" in f and "nproc" in f
    assert list(inspect.signature(sg.SourceFinder.__call__).parameters) == ["self", "data",
                                                                          "threshold", "mask"]
    s = inspect.signature(sg.source_info).parameters
    assert s["deblend"].default is False and s["nlevels"].default == 32
    assert s["contrast"].default == 0.001
    assert sg.DEBLEND_MAX_BOX >= 4096


def test_c_abi_argument_checks(sg):
    import _bsgp
    L = _bsgp.lib()
    assert "bsgp_deblend_sources" in _bsgp.EXPORTED
    p = 8  # a non-NULL pointer that is never followed: the checks come first

    def call(npixels=1, nlevels=32, contrast=0.001, mode=1, conn=8, out=16):
        return L.bsgp_deblend_sources(p, p, 1, 4, 4, 1, p, p, None, npixels, nlevels, contrast, mode,
                                      conn, out, p, p, None)

    for kw, word in ((dict(nlevels=0), b"nlevels"), (dict(contrast=1.5), b"contrast"),
                     (dict(contrast=-0.5), b"contrast"), (dict(npixels=0), b"npixels"),
                     (dict(conn=5), b"connectivity"), (dict(mode=2), b"mode"), (dict(out=p), b"labels_out")):
        assert call(**kw) == _bsgp.BSGP_ERR_ARG and word in L.bsgp_last_error(), kw


def test_numbering_rule(sg):
    """D7: parents left as they are first, in input order, then the children
    by parent; absent labels get no number."""
    base, n = sg.deblend_numbering([0, 3, 0, 2, 0])
    assert list(base) == [1, 4, 2, 7, 3] and n == 8
    base, n = sg.deblend_numbering([0, 3, 0, 2, 0], present=[1, 1, 0, 1, 1])
    assert list(base) == [1, 3, 0, 6, 2] and n == 7
    base, n = sg.deblend_numbering([])
    assert len(base) == 0 and n == 0


def test_fixture_is_consistent_with_seg_cases(sg, fx, seg):
    for tag, src in (("s1", "s1_lab5"), ("s2", "s2_lab5"), ("app5", "app_lab5"), ("app1", "app_lab1")):
        lab, out, par = seg[src].astype(np.int64), fx[f"{tag}_out"].astype(np.int64), fx[f"{tag}_parent"]
        assert np.array_equal(out != 0, lab != 0)  # no pixel dropped or added
        assert len(par) == out.max() + 1 and np.array_equal(par[out], lab)
        areas = np.bincount(lab.ravel())[1:]
        assert np.array_equal(np.bincount(par[out.ravel()][out.ravel() > 0])[1:], areas)
        nchild = np.bincount(par[1:], minlength=lab.max() + 1)[1:]
        base, n = sg.deblend_numbering(np.where(nchild > 1, nchild, 0))
        assert n == out.max()
        for l in range(1, lab.max() + 1):  # D7 on the fixture's own parents
            assert set(np.unique(out[lab == l])) == set(range(base[l - 1], base[l - 1] + nchild[l - 1]))
    assert (fx["s1_out"].max(), fx["s2_out"].max()) == (10, 7)
    assert (fx["app5_out"].max(), fx["app1_out"].max()) == (104, 647)
    for l in (3, 5, 438, 417, 47):
        box = np.argwhere(seg["app_lab1"] == l)
        assert fx[f"crop{l}_mask"].shape == tuple(box.max(0) - box.min(0) + 1)
        assert fx[f"crop{l}_mask"].sum() == len(box)
    assert [int(fx[f"crop{l}_out"].max()) for l in (3, 5, 438, 417, 47)] == [18, 6, 2, 2, 8]


def test_restatement_reproduces_the_fixture(fx, seg):
    """tests/deblend_ref.py with its serial flood (the device's tie rule) gives
    the fixture's images, which the generator wrote with skimage's watershed."""
    out, par, st = deblend_ref.deblend(seg["s1_conv"], seg["s1_lab5"], 5)
    assert np.array_equal(out, fx["s1_out"]) and np.array_equal(par, fx["s1_parent"])
    assert st["nsplit"] == 1 and st["nchildren"] == 3
    out, par, st = deblend_ref.deblend(fx["crop5_conv"], fx["crop5_mask"].astype(np.int32), 1)
    assert np.array_equal(out, fx["crop5_out"]) and st["removals"] == 3
