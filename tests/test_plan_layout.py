"""The plan layout on the host (no GPU): bsgp_plan_layout, the diagnostic entry
point over plan_layout (csrc/bsgp_layout.hpp), gives what plan creation uses.

The expected values were printed by a stand-alone program holding a verbatim
copy of the arithmetic bsgp_plan_create_checked had before plan_layout was
extracted from it; they are not the new code's output.  The flagship case is
also SGeo256's compile-time constants (csrc/bsgp_device.hpp): a drift between
the two would silently drop the static-geometry path on the GPU."""
import ctypes

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

LIN, CIRC, F64, F32 = 1, 0, 0, 1
FIELDS = ["H", "W", "P", "Q", "Qh", "sld", "lpad", "nfw", "nfc", "coop", "tw2", "twmix",
          "fp_lds_tw", "fq_lds_tw", "fp_lds_tw2", "fq_lds_tw2", "lds_fft_bytes", "lds_bytes",
          "wg_per_cu", "vec_stride", "spec_off", "slot_stride", "fp_ns", "fq_ns"]
NVAL = len(FIELDS) + 2 * 16


def _layout(H, W, kh, kw, mode, storage, n=NVAL):
    import _bsgp
    L = _bsgp.lib()
    L.bsgp_plan_layout.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_void_p, ctypes.c_int32]
    out = np.full(NVAL, -7, np.int64)
    rc = L.bsgp_plan_layout(H, W, kh, kw, mode, storage, out.ctypes.data, n)
    return rc, out, L.bsgp_last_error().decode()


def _pad(r):
    return list(r) + [0] * (16 - len(r))


# (H, W, kh, kw, conv_mode, storage): the 24 fields, P's radices, Q's radices
R270, R400, R480, R2048 = [2, 3, 3, 3, 5], [4, 4, 5, 5], [4, 4, 2, 3, 5], [4, 4, 4, 4, 4, 2]
CASES = {
    # the flagship: SGeo256
    (256, 256, 25, 25, LIN, F64): ([256, 256, 270, 270, 136, 256, 273, 4, 4, 0, 0, -1,
                                    36224, 36224, -1, -1, 34944, 40544, 4, 65536, 589824, 790528,
                                    5, 5], R270, R270),
    # the application tiles on the 400- and 480-point grids
    (375, 375, 25, 25, LIN, F64): ([375, 375, 400, 400, 201, 376, 403, 4, 4, 0, 0, -1,
                                    52864, 52864, -1, -1, 51584, 59264, 2, 140640, 1265760,
                                    1698208, 4, 4], R400, R400),
    (450, 450, 25, 25, LIN, F64): ([450, 450, 480, 480, 241, 450, 483, 4, 4, 0, 0, -1,
                                    63104, 63104, -1, -1, 61824, 70784, 2, 202528, 1822752,
                                    2444736, 5, 5], R480, R480),
    # a 2048 x 2048 grid: cooperative, two thread groups, two-level twiddles in LDS
    (2030, 2030, 25, 25, LIN, F64): ([2030, 2030, 2048, 2048, 1025, 2030, 2051, 2, 1, 1, 10752,
                                      1536, -1, -1, 0, 0, 131264, 144064, 1, 4120928, 37088352,
                                      49491712, 6, 6], R2048, R2048),
    # only the columns / only the rows have 2048 points
    (2036, 300, 25, 25, LIN, F64): ([2036, 300, 2048, 320, 161, 2036, 2049, 2, 1, 1, 10752, 1536,
                                     -1, -1, 0, -1, 131136, 143936, 1, 610816, 5497344, 7374592,
                                     6, 4], R2048, [4, 4, 4, 5]),
    (300, 2036, 25, 25, LIN, F64): ([300, 2036, 320, 2048, 1025, 300, 2051, 2, 1, 1, 1536, -1,
                                     -1, -1, -1, 0, 131264, 134848, 1, 610816, 5497344, 7333984,
                                     4, 6], [4, 4, 4, 5], R2048),
    # cooperative, one group, no LDS twiddles
    (2040, 2040, 25, 25, LIN, F64): ([2040, 2040, 2160, 2160, 1081, 2040, 2163, 1, 1, 1, 0, -1,
                                      -1, -1, -1, -1, 69216, 71264, 2, 4161600, 37454400,
                                      50188096, 6, 6], [4, 4, 3, 3, 3, 5], [4, 4, 3, 3, 3, 5]),
    # a star stamp
    (31, 31, 25, 25, LIN, F64): ([31, 31, 45, 45, 23, 32, 47, 4, 4, 0, 0, -1, 7296, 7296, -1, -1,
                                  6016, 8016, 4, 992, 8928, 12384, 3, 3], [3, 3, 5], [3, 3, 5]),
    # circular
    (64, 64, 64, 64, CIRC, F64): ([64, 64, 64, 64, 33, 64, 67, 4, 4, 0, 0, -1, 9856, 9856, -1, -1,
                                   8576, 10880, 4, 4096, 36864, 49280, 3, 3], [4, 4, 4], [4, 4, 4]),
    # float32 storage: the slot shrinks, nothing else moves
    (256, 256, 25, 25, LIN, F32): ([256, 256, 270, 270, 136, 256, 273, 4, 4, 0, 0, -1,
                                    36224, 36224, -1, -1, 34944, 40544, 4, 65536, 360448, 561152,
                                    5, 5], R270, R270),
    # the two plans of tests/test_gpu_abi.py::test_plan_info_is_plan_layout
    (16, 16, 5, 5, LIN, F64): ([16, 16, 18, 18, 10, 16, 21, 4, 4, 0, 0, -1, 3968, 3968, -1, -1,
                                2688, 4256, 4, 256, 2304, 3136, 3, 3], [2, 3, 3], [2, 3, 3]),
    (16, 16, 16, 16, CIRC, F64): ([16, 16, 16, 16, 9, 16, 19, 4, 4, 0, 0, -1, 3712, 3712, -1, -1,
                                   2432, 3968, 4, 256, 2304, 3104, 2, 2], [4, 4], [4, 4]),
}
# with a knob set, on the shape where it changes the result
KNOB_CASES = {
    # no twiddle condition: 375^2 takes three workgroups per CU, twiddles from global memory
    ("BSGP_PERWAVE_TW", "0", 375): ([375, 375, 400, 400, 201, 376, 403, 4, 4, 0, 0, -1,
                                     -1, -1, -1, -1, 51584, 52864, 3, 140640, 1265760, 1698208,
                                     4, 4], R400, R400),
    # one load batch per thread: the 2048-point rows stay on one group, two workgroups per CU
    ("BSGP_COOP_ELEMS", "4", 2030): ([2030, 2030, 2048, 2048, 1025, 2030, 2051, 1, 1, 1, 10752,
                                      1536, -1, -1, 0, 0, 65632, 78432, 2, 4120928, 37088352,
                                      49491712, 6, 6], R2048, R2048),
    # per-wave plans only at four per CU: 375^2 goes cooperative, four thread groups
    ("BSGP_PERWAVE_MIN_WG", "4", 375): ([375, 375, 400, 400, 201, 376, 403, 4, 4, 1, 0, -1,
                                         -1, -1, -1, -1, 51584, 53632, 3, 140640, 1265760,
                                         1698208, 4, 4], R400, R400),
}


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("BSGP_PERWAVE_MIN_WG", "BSGP_PERWAVE_TW", "BSGP_COOP_ELEMS"):
        monkeypatch.delenv(k, raising=False)


def _check(got, want):
    fields, rp, rq = want
    exp = list(fields) + _pad(rp) + _pad(rq)
    names = FIELDS + [f"fp_radix{i}" for i in range(16)] + [f"fq_radix{i}" for i in range(16)]
    diff = {n: (int(g), e) for n, g, e in zip(names, got, exp) if g != e}
    assert not diff, diff


@pytest.mark.parametrize("args", list(CASES), ids=lambda a: "x".join(map(str, a)))
def test_layout_is_the_parents(args):
    rc, out, err = _layout(*args)
    assert rc == 0, err
    _check(out, CASES[args])


@pytest.mark.parametrize("knob", list(KNOB_CASES), ids=lambda k: f"{k[0]}={k[1]}")
def test_layout_knobs(knob, monkeypatch):
    name, value, H = knob
    monkeypatch.setenv(name, value)
    rc, out, err = _layout(H, H, 25, 25, LIN, F64)
    assert rc == 0, err
    _check(out, KNOB_CASES[knob])
    # a value outside the knob's range is ignored
    monkeypatch.setenv(name, "99")
    rc, out, err = _layout(H, H, 25, 25, LIN, F64)
    assert rc == 0, err
    _check(out, CASES[(H, H, 25, 25, LIN, F64)])


def test_flagship_is_sgeo256():
    """SGeo256's constants (bsgp_device.hpp), as literals: what static_geo_plan
    compares the plan with at run time."""
    rc, out, err = _layout(256, 256, 25, 25, LIN, F64)
    assert rc == 0, err
    g = dict(zip(FIELDS, map(int, out)))
    assert (g["P"], g["Q"], g["Qh"], g["sld"], g["lpad"]) == (270, 270, 136, 256, 273)
    assert (g["coop"], g["nfw"], g["nfc"], g["wg_per_cu"]) == (0, 4, 4, 4)
    assert (g["tw2"], g["twmix"]) == (0, -1)
    assert g["lds_fft_bytes"] == 34944
    assert (g["fp_lds_tw"], g["fq_lds_tw"]) == (36224, 36224)
    assert g["lds_bytes"] == 40544


def test_over_the_lds_limit():
    import _bsgp
    rc, out, err = _layout(5000, 5000, 25, 25, LIN, F64)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED
    assert err == "FFT length too large for one workgroup's LDS"
    assert (out == -7).all()


def test_arguments():
    import _bsgp
    for bad in [(0, 8, 3, 3, LIN, F64), (8, 8, 0, 3, LIN, F64), (8, 8, 3, 3, 2, F64),
                (8, 8, 3, 3, LIN, 7), (8, 8, 3, 3, CIRC, F64)]:
        rc, out, err = _layout(*bad)
        assert rc == _bsgp.BSGP_ERR_ARG and err, bad
    L = _bsgp.lib()
    assert L.bsgp_plan_layout(8, 8, 3, 3, LIN, F64, None, 4) == _bsgp.BSGP_ERR_ARG
    # only the first n values are written
    rc, out, err = _layout(8, 8, 3, 3, LIN, F64, n=4)
    assert rc == 0 and list(out[:4]) == [8, 8, 9, 9] and (out[4:] == -7).all()


def test_invariants_over_a_sweep():
    """Every regime: per-wave at four and two workgroups per CU, cooperative
    with two groups and with one."""
    seen = set()
    sizes = list(range(16, 520, 9)) + [600, 800, 1012, 1013, 1500, 2014, 2030, 2036, 2037, 2100]
    for H in sizes:
        rc, out, err = _layout(H, H, 25, 25, LIN, F64)
        assert rc == 0, (H, err)
        g = dict(zip(FIELDS, map(int, out)))
        seen.add((g["coop"], g["nfw"], g["wg_per_cu"]))
        assert g["lds_bytes"] <= 160 * 1024 // g["wg_per_cu"] - 256, (H, g)
        assert 1 <= g["nfc"] <= g["nfw"], (H, g)
        assert g["coop"] or g["nfw"] == 4, (H, g)
        assert g["sld"] % 2 == 0 and g["sld"] >= H, (H, g)
        assert g["slot_stride"] % 32 == 0, (H, g)
    assert {(0, 4, 4), (0, 4, 2), (1, 2, 1), (1, 1, 2)} <= seen, seen
