"""Host-side checks of the star-stamp cutouts and selection: the
argument checks, the restated box rule against astropy's own cutouts, the
header's declarations and the binding's constants.  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

import starstamps_ref as ref


def test_check_cutout_args_rejections():
    import stamps
    ok = stamps.check_cutout_args((48, 64), [[1.5, 2.0], [np.nan, 3.0]], 31)
    assert ok[0] == (48, 64) and ok[1].shape == (2, 2) and ok[1].dtype == np.float64
    assert ok[2] == (31, 31)
    assert stamps.check_cutout_args((48, 64), [], (30, 31))[1].shape == (0, 2)
    assert stamps.check_cutout_args((48, 64), np.zeros((0, 2)), np.int64(5))[2] == (5, 5)
    for shape in [(48,), (2, 48, 64), (0, 64)]:
        with pytest.raises(ValueError, match="image must be"):
            stamps.check_cutout_args(shape, [[1, 2]], 31)
    for pos in [[1.0, 2.0], [[1.0, 2.0, 3.0]], np.zeros((2, 2, 2)), np.zeros((0, 3))]:
        with pytest.raises(ValueError, match=r"positions must be \[n, 2\]"):
            stamps.check_cutout_args((48, 64), pos, 31)
    with pytest.raises(ValueError, match="positions must be numbers"):
        stamps.check_cutout_args((48, 64), [["a", "b"]], 31)
    for size in [31.0, (31,), (31, 31, 31), (31, 2.5), True, "31", None]:
        with pytest.raises(ValueError, match="size must be an int or a pair"):
            stamps.check_cutout_args((48, 64), [[1, 2]], size)
    for size in [0, (31, -1)]:
        with pytest.raises(ValueError, match="size must be positive"):
            stamps.check_cutout_args((48, 64), [[1, 2]], size)
    with pytest.raises(ValueError, match="a cutout holds at most"):
        stamps.check_cutout_args((48, 64), [[1, 2]], (4097, 4096))


def test_box_rule_reproduces_astropy_cutouts():
    """The restated rule gives astropy 4.3.1's Cutout2D data at the centres
    tests/golden/make_golden_io.py used: the middles of the golden boxes."""
    g = golden("ref_cutouts.npz")
    b = g["boxes"].astype(np.float64)
    centres = np.stack(((b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2), axis=1)
    out, box, st = ref.cutout_ref(g["img"], centres, tuple(int(v) for v in g["shape"]))
    assert not st.any()
    np.testing.assert_array_equal(box, g["boxes"])
    assert out.dtype == g["cutouts"].dtype and out.tobytes() == g["cutouts"].tobytes()


def test_box_rule_edges():
    assert [ref.box_min(x, 31) for x in (20.49, 20.5, 20.51, 15.0, 14.99, 14.5)] == [5, 5, 6, 0, 0, -1]
    assert ref.box_min(1e300, 31) == ref.BOX_LIMIT and ref.box_min(-1e300, 31) == -ref.BOX_LIMIT
    img = np.arange(12.0).reshape(3, 4)
    out, box, st = ref.cutout_ref(img, [[0.0, 0.0], [-20.0, 1.0], [np.nan, 1.0], [2.0, 1.5]], (3, 4))
    import _bsgp as B
    assert st.tolist() == [B.BSGP_STAMP_PARTIAL, B.BSGP_STAMP_NO_OVERLAP,
                           B.BSGP_STAMP_BAD_POSITION, 0]
    assert box.tolist() == [[-2, -1, 2, 2], [-22, 0, -18, 3], [0, 0, 0, 0], [0, 0, 4, 3]]
    np.testing.assert_array_equal(out[0], [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 4, 5]])
    assert not out[1].any() and not out[2].any()
    np.testing.assert_array_equal(out[3], img)


def test_header_and_binding_agree():
    import _bsgp as B
    txt = open(os.path.join(ROOT, "include", "bsgp.h")).read()
    for fn in ("bsgp_extract_stamps", "bsgp_stamp_select"):
        assert re.search(rf"^int {fn}\(", txt, flags=re.M), fn
        assert fn in B.EXPORTED
    defs = dict(re.findall(r"^#define (BSGP_STAMP_\w+) (\d+)$", txt, flags=re.M))
    assert set(defs) == {"BSGP_STAMP_PARTIAL", "BSGP_STAMP_NO_OVERLAP", "BSGP_STAMP_BAD_POSITION",
                         "BSGP_STAMP_NO_SOURCE", "BSGP_STAMP_MULTI_SOURCE", "BSGP_STAMP_BAD_FLUX",
                         "BSGP_STAMP_NO_CANDIDATE", "BSGP_STAMP_RESTORED_NO_SOURCE",
                         "BSGP_STAMP_ROW_COLS"}
    for name, val in defs.items():
        assert getattr(B, name) == int(val), name
    bits = [int(v) for k, v in defs.items() if k != "BSGP_STAMP_ROW_COLS"]
    assert sorted(bits) == [1 << i for i in range(8)]
    import stamps
    assert len(stamps.ROW_COLUMNS) == B.BSGP_STAMP_ROW_COLS


def test_select_restatement_rule():
    """The restatement itself on a hand-made case: first of equal scores, NaN
    never, an undetected candidate is +inf, none below +inf gives -1."""
    obs = np.zeros((2, 1, 8))
    obs[:, 0, :] = [100.0, 0, 0, 15.0, 15.5, 2.0, 0.1, 1.5]
    res = np.zeros((6, 1, 8))
    res[:, 0, :] = [90.0, 0, 0, 15.0, 15.5, 1.0, 0.0, 1.0]
    res[0, 0, 0], res[1, 0, 0], res[2, 0, 0] = np.nan, 95.0, 95.0
    nl = np.array([1, 1, 1, 0, 0, 0])
    sc, best, rows, nit, st = ref.select_ref(nl, res, obs, np.arange(6) + 10, 3)
    assert best.tolist() == [1, -1] and nit.tolist() == [11, -1]
    import _bsgp as B
    assert st.tolist() == [0, B.BSGP_STAMP_NO_CANDIDATE]
    assert np.isnan(sc[0, 0]) and sc[0, 1] == sc[0, 2] == 1 - 95.0 / 100.0
    assert np.all(np.isinf(sc[1])) and np.all(np.isnan(rows[1, [1, 2, 3, 4, 8, 9, 10]]))
    assert rows[0, 0] == 100.0 and rows[0, 1] == 95.0 and rows[1, 0] == 100.0
