"""Host-side checks of the global-memory deblending path (no device): the
fixture tests/golden/deblend_large_cases.npz reproduces itself through
tests/deblend_ref.py, the new keywords are checked before the device is
touched, and ``bsgp_deblend_sources_large`` is in the header, the ctypes
binding and the built library."""
import inspect
import os
import re

import numpy as np
import pytest

import deblend_ref
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sg():
    import segmentation
    return segmentation


@pytest.fixture(scope="module")
def fx():
    return golden("deblend_large_cases.npz")


@pytest.mark.parametrize("tag,nchild,removals", (("big", 16, 0), ("small", 14, 1)))
def test_fixture_reproduces_itself(sg, fx, tag, nchild, removals):
    d, m = fx[f"{tag}_conv"], fx[f"{tag}_mask"]
    assert m.size > sg.DEBLEND_MAX_BOX and 10 <= m.sum() <= sg.DEBLEND_LARGE_MAX_AREA
    assert m.any(0).all() and m.any(1).all()  # the crop is the parent's box
    out, par, st = deblend_ref.deblend(d, m.astype(np.int32), 5)  # raises on a tie margin
    assert np.array_equal(out, fx[f"{tag}_out"]) and np.array_equal(par, fx[f"{tag}_parent"])
    assert (st["nsplit"], st["nchildren"], st["removals"]) == (1, nchild, removals)
    assert np.array_equal(out != 0, m)


def test_keyword_checks_raise_before_the_device(sg):
    d, lab = np.ones((6, 7)), np.ones((6, 7), np.int32)
    for bad in (-1, sg.DEBLEND_MAX_BOX + 1, 2.5, True, "0"):
        with pytest.raises((ValueError, TypeError), match="lds_max_box"):
            sg.deblend_sources(d, lab, 1, large_parents=True, lds_max_box=bad)
    with pytest.raises(ValueError, match="needs large_parents=True"):
        sg.deblend_sources(d, lab, 1, lds_max_box=0)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="large_parents must be a bool"):
            sg.deblend_sources(d, lab, 1, large_parents=bad)
        with pytest.raises(ValueError, match="large_parents must be a bool"):
            sg.SourceFinder(5, large_parents=bad)
        with pytest.raises(ValueError, match="large_parents must be a bool"):
            sg.source_info(d, 3, deblend=True, large_parents=bad)
    # the earlier checks still come first and still hold with the new keywords
    with pytest.raises(ValueError, match="sinh"):
        sg.deblend_sources(d, lab, 1, mode="sinh", large_parents=True, lds_max_box=0)
    sg.check_deblend_args((6, 7), (6, 7), 1, large_parents=True, lds_max_box=0)
    sg.check_deblend_args((6, 7), (6, 7), 1, large_parents=True, lds_max_box=sg.DEBLEND_MAX_BOX)
    sg.check_deblend_args((6, 7), (6, 7), 1, lds_max_box=sg.DEBLEND_MAX_BOX)


def test_signatures_and_constants(sg):
    import _bsgp
    p = inspect.signature(sg.deblend_sources).parameters
    assert p["large_parents"].default is False and p["lds_max_box"].default == sg.DEBLEND_MAX_BOX
    assert inspect.signature(sg.SourceFinder.__init__).parameters["large_parents"].default is False
    assert inspect.signature(sg.source_info).parameters["large_parents"].default is False
    assert sg.DEBLEND_LARGE_MAX_AREA == _bsgp.BSGP_DEBLEND_LARGE_MAX_AREA == 262144
    assert sg.DEBLEND_LARGE_MAX_AREA >= 450 * 450 and sg.DEBLEND_LARGE_MAX_AREA >= 512 * 512
    with open(os.path.join(ROOT, "include", "bsgp.h")) as f:
        head = f.read()
    assert re.search(r"#define BSGP_DEBLEND_LARGE_MAX_AREA 262144\b", head)
    assert re.search(r"#define BSGP_DEBLEND_MAX_BOX 4096\b", head)


def test_symbol_in_header_binding_and_library(sg):
    import _bsgp
    with open(os.path.join(ROOT, "include", "bsgp.h")) as f:
        head = f.read()
    m = re.search(r"int bsgp_deblend_sources_large\(([^;]*)\);", head)
    assert m, "bsgp_deblend_sources_large is not declared in include/bsgp.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    old = re.search(r"int bsgp_deblend_sources\(([^;]*)\);", head).group(1)
    old = [a.strip() for a in old.replace("\n", " ").split(",")]
    assert args[:14] == old[:14] and args[14] == "int32_t lds_max_box" and args[15:] == old[14:]
    assert "bsgp_deblend_sources_large" in _bsgp.EXPORTED
    L = _bsgp.lib()
    fn = L.bsgp_deblend_sources_large  # AttributeError if the built library lacks it
    assert len(fn.argtypes) == len(args) == len(L.bsgp_deblend_sources.argtypes) + 1


def test_c_abi_argument_checks(sg):
    import _bsgp
    L = _bsgp.lib()
    p = 8  # a non-NULL pointer that is never followed: the checks come first

    def call(lds=0, nlevels=32, out=16):
        return L.bsgp_deblend_sources_large(p, p, 1, 4, 4, 1, p, p, None, 1, nlevels, 0.001, 1, 8,
                                            lds, out, p, p, None)

    for kw, word in ((dict(lds=-1), b"lds_max_box"), (dict(lds=_bsgp.BSGP_DEBLEND_MAX_BOX + 1), b"lds_max_box"),
                     (dict(nlevels=0), b"nlevels"), (dict(out=p), b"labels_out")):
        assert call(**kw) == _bsgp.BSGP_ERR_ARG and word in L.bsgp_last_error(), kw
