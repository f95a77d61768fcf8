"""Source validation, CPU side: sanity cases of the numpy
restatement (tests/validate_ref.py), the host-only argument checks, the
window cap against the header, and the leaf plan of numpy's pairwise sum
(csrc/bsgp_validate.hpp) against np.sum."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _bsgp
import segmentation
from conftest import ROOT
from segmentation import VALIDATE_MAX, check_validate_args, validate_sources, validation_source
from validate_ref import validate_one, validate_ref, window

CSRC = os.path.join(ROOT, "beta-sgp_amd", "csrc")


# ---------------------------------------------------------------- restatement
def test_ref_hand_computed_3x3():
    """size 3 at (2, 2) of a 5 x 5 frame: the window is rows and columns 1..3."""
    img = np.arange(25, dtype=np.float64).reshape(5, 5)
    bkg = np.array([[0, 0, 0, 0, 0],
                    [0, 1, 2, 3, 0],
                    [0, 4, 50, 6, 0],
                    [0, 7, 8, 9, 0],
                    [0, 0, 0, 0, 0]], dtype=np.float64)
    rms = np.full((5, 5), 0.5)
    valid, sp, b, r, st = validate_one(img, (2.0, 2.0), bkg, rms, size=3)
    assert sp == (16.0 + 17.0 + 18.0) / 3 == 17.0
    assert b == 6.0  # of 1 2 3 4 6 7 8 9 50
    assert r == 0.5 and st == 0
    assert valid is True  # 17 > 6 + 1.5
    valid, sp, b, r, st = validate_one(img, (2.0, 2.0), bkg + 10.0, rms, size=3)
    assert b == 16.0 and valid is False  # 17 > 17.5 is false
    # the box rule: ceil(pos - size / 2) -- 2.5 starts the box at 1, 2.6 at 2
    np.testing.assert_array_equal(window(img, 1, 1, 3, 3), img[1:4, 1:4])
    assert validate_one(img, (2.5, 2.0), bkg, rms, size=3)[1] == 17.0
    assert validate_one(img, (2.6, 2.0), bkg, rms, size=3)[1] == (17.0 + 18.0 + 19.0) / 3
    # an even window of 4 values: the median is the mean of the two middle ones
    assert validate_one(img, (2.0, 2.0), bkg, rms, size=2)[2] == (2.0 + 4.0) / 2  # of 1 2 4 50


def test_ref_fill_region():
    """A box that only touches the frame's corner pixel: 8 of 9 cells are fill,
    which takes part; a box wholly outside is NO_OVERLAP, a NaN BAD_POSITION."""
    img = np.full((6, 6), 9.0)
    bkg, rms = np.full((6, 6), 4.0), np.full((6, 6), 1.0)
    valid, sp, b, r, st = validate_one(img, (-1.0, -1.0), bkg, rms, size=3)
    assert st == _bsgp.BSGP_STAMP_PARTIAL
    assert sp == (0.0 + 0.0 + 9.0) / 3 and b == 0.0 and r == 1.0 / 9
    assert valid is True  # 3 > 0 + 3 / 9
    valid, sp, b, r, st = validate_one(img, (-2.0, 3.0), bkg, rms, size=3)  # box x: -3 .. -1
    assert st == _bsgp.BSGP_STAMP_NO_OVERLAP and valid is False
    assert np.isnan(sp) and np.isnan(b) and np.isnan(r)
    for bad in (np.nan, np.inf, -np.inf):
        valid, sp, b, r, st = validate_one(img, (bad, 3.0), bkg, rms, size=3)
        assert st == _bsgp.BSGP_STAMP_BAD_POSITION and valid is False and np.isnan(sp)


def test_ref_strict_at_equality():
    img = np.full((8, 8), 2.5)
    bkg, rms = np.full((8, 8), 1.0), np.full((8, 8), 0.5)
    assert validate_one(img, (4.0, 4.0), bkg, rms, size=4)[:4] == (False, 2.5, 1.0, 0.5)
    img[4, 4] = img[4, 3] = img[3, 3] = np.nextafter(2.5, 3.0)
    assert validate_one(img, (4.0, 4.0), bkg, rms, size=4)[0] is True
    out = validate_ref(img, [(4.0, 4.0), (np.nan, 0.0)], bkg, rms, size=4)
    assert out["valid"].tolist() == [True, False] and out["stats"].shape == (2, 3)
    # a NaN in a window makes its statistic NaN and the source invalid
    for k in range(3):
        frames = [img.copy(), bkg.copy(), rms.copy()]
        frames[k][4, 4] = np.nan
        res = validate_one(frames[0], (4.0, 4.0), frames[1], frames[2], size=4)
        assert res[0] is False and np.isnan(res[1 + k])


# ---------------------------------------------------------------- arguments
def test_check_validate_args_raises_without_gpu():
    ok = ((160, 144), (160, 144), (160, 144))
    assert check_validate_args(*ok) == (100, 100)
    assert check_validate_args(*ok, size=(9, 14)) == (9, 14)
    assert check_validate_args((3, 160, 144), (160, 144), (160, 144), 128) == (128, 128)
    assert check_validate_args((3, 160, 144), (3, 160, 144), (3, 160, 144), 7,
                               positions_shape=[(0, 2), (5, 2), (17, 2)]) == (7, 7)
    bad = [
        dict(a=((160,), (160,), (160,))),                                  # not an image
        dict(a=((160, 144), (160, 143), (160, 143))),                      # map shape
        dict(a=((160, 144), (160, 144), (144, 160))),                      # rms shape
        dict(a=((160, 144), (2, 160, 144), (2, 160, 144))),                # batch of maps, one image
        dict(a=((3, 160, 144), (2, 160, 144), (2, 160, 144))),             # B differs
        dict(a=((3, 160, 144), (3, 160, 144), (160, 144))),                # maps differ
        dict(a=ok, size=0), dict(a=ok, size=-3), dict(a=ok, size=2.5), dict(a=ok, size=(3, 0)),
        dict(a=ok, size=(3, 3, 3)), dict(a=ok, size=True),
        dict(a=ok, size=129), dict(a=ok, size=(128, 129)),                 # n > VALIDATE_MAX
        dict(a=ok, nsigma=float("nan")), dict(a=ok, nsigma="3"),
        dict(a=ok, positions_shape=(5,)), dict(a=ok, positions_shape=(5, 3)),
        dict(a=ok, positions_shape=(2, 5, 2)), dict(a=ok, positions_shape=[(5, 2)]),
        dict(a=((3, 160, 144), (160, 144), (160, 144)), positions_shape=(5, 2)),
        dict(a=((3, 160, 144), (160, 144), (160, 144)), positions_shape=[(5, 2), (5, 2)]),
    ]
    for kw in bad:
        a = kw.pop("a")
        with pytest.raises(ValueError):
            check_validate_args(*a, **kw)


def test_entry_points_check_before_any_gpu_use():
    """The public calls raise ValueError for a bad argument even where no GPU
    is visible: the checks run first (a BsgpError would mean the device was
    asked for)."""
    img, m = np.zeros((16, 12)), np.ones((16, 12))
    with pytest.raises(ValueError, match="VALIDATE_MAX"):
        validate_sources(img, [[3.0, 4.0]], m, m, size=129)
    with pytest.raises(ValueError, match="size"):
        validation_source(img, (3.0, 4.0), m, m, size=0)
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        validate_sources(img, np.zeros((4, 3)), m, m)
    with pytest.raises(ValueError, match="rmsmap"):
        validate_sources(img, np.zeros((4, 2)), m, np.ones((16, 13)))
    with pytest.raises(ValueError, match="list of 2"):
        validate_sources(np.zeros((2, 16, 12)), np.zeros((4, 2)), m, m)
    with pytest.raises(ValueError, match="VALIDATE_MAX"):
        segmentation.source_info(img, 4, validate=True, validate_size=200)
    sig = inspect.signature(validation_source)
    assert list(sig.parameters) == ["image", "coord", "bkgmap", "rmsmap", "size"]
    assert sig.parameters["size"].default == 100
    sig = inspect.signature(validate_sources)
    assert list(sig.parameters) == ["image", "positions", "bkgmap", "rmsmap", "size", "nsigma",
                                    "device_out"]
    assert sig.parameters["nsigma"].default == 3.0 and sig.parameters["size"].default == 100
    si = inspect.signature(segmentation.source_info).parameters
    assert si["validate"].default is False and si["validate_size"].default == 100


def test_c_entry_reports_argument_errors_without_a_device():
    L = _bsgp.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    ok = dict(image=p, dtype=1, bkg=p, rms=p, B=1, H=4, W=4, per=0, xy=p, stride=2, n=None, cap=1,
              sh=2, sw=2, nsigma=3.0, stats=p, valid=p, status=p, stream=None)

    def call(**kw):
        return L.bsgp_validate_sources(*{**ok, **kw}.values())

    assert call(sh=129, sw=128) == _bsgp.BSGP_ERR_UNSUPPORTED
    assert b"16384" in L.bsgp_last_error()
    for kw in (dict(dtype=7), dict(H=0), dict(sw=0), dict(stride=1), dict(cap=-1), dict(B=-1),
               dict(nsigma=float("nan")), dict(image=None), dict(rms=None), dict(xy=None),
               dict(valid=None)):
        assert call(**kw) == _bsgp.BSGP_ERR_ARG, kw
    assert call(B=0, image=None) == 0 and call(cap=0, xy=None) == 0  # no-ops follow no pointer


def test_validate_max_is_the_headers():
    txt = open(os.path.join(ROOT, "include", "bsgp.h")).read()
    assert int(re.search(r"#define BSGP_VALIDATE_MAX (\d+)", txt).group(1)) == VALIDATE_MAX == 16384
    assert _bsgp.BSGP_VALIDATE_MAX == VALIDATE_MAX


# ---------------------------------------------------------------- leaf plan
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = tmp_path_factory.mktemp("validate_plan") / "libvalidate_plan.so"
    # -ffp-contract=off: the same rounding as the gfx950 build
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "validate_plan.cpp"), "-o", str(so)],
                   check=True)
    L = ctypes.CDLL(str(so))
    L.vp_sum.restype = L.vp_sum_recursive.restype = ctypes.c_double
    L.vp_sum.argtypes = L.vp_sum_recursive.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.vp_leaves.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return L


@pytest.mark.parametrize("n", [1, 7, 8, 128, 129, 144, 10000, 16384])
def test_leaf_plan_sums_like_numpy(plan, n):
    rng = np.random.default_rng(n)
    for trial in range(8):
        # magnitudes over 40 binades and both signs: every addition rounds, so
        # another order of the additions gives other bits
        a = rng.uniform(-1.0, 1.0, n) * np.exp2(rng.uniform(-20.0, 20.0, n))
        if trial == 0:
            a = np.abs(a)  # the rms case: non-negative
        want = np.sum(a)
        assert plan.vp_sum(a.ctypes.data, n) == want
        if n <= 8192:  # one buffer of numpy's reduction: the recursion alone
            assert plan.vp_sum_recursive(a.ctypes.data, n) == want
        assert np.mean(a.reshape(-1, 1 if n % 2 else 2)) == want / n  # V4: a contiguous 2-D window
    off, ln = np.zeros(256, np.int32), np.zeros(256, np.int32)
    nl = plan.vp_leaves(n, off.ctypes.data, ln.ctypes.data, 256)
    assert 1 <= nl <= 256 and (nl == 1) == (n <= 128)
    assert off[0] == 0 and np.array_equal(off[1:nl], np.cumsum(ln[:nl])[:-1]) and ln[:nl].sum() == n
    assert ln[:nl].max() <= 128
    if n == 144:  # the left half is a multiple of 8: 72, 72
        assert ln[:nl].tolist() == [72, 72]


def test_leaf_plan_fits_one_leaf_per_thread(plan):
    """Every n up to the cap: the leaves tile the window and there are at most
    256 of them, one per thread of the workgroup."""
    most = plan.vp_check_upto(VALIDATE_MAX)
    assert 0 < most <= plan.vp_max_leaves() == 256, most
