"""The exact operator reference (tests/op_ref.py) against numpy's float64 FFT
operators and the golden linear convolutions, and the sweep table against
plan_layout: every row must be in the branch it is listed for, so that a
change of plan_layout cannot silently thin the device sweep
(tests/test_gpu_opsweep.py).  No GPU.

REF_TOL: numpy's operator differs from the exact sums by at most 8.8e-16 in
either norm over 14 shapes from 7 x 11 to 375 x 375 (the worst: a dense
31 x 31 kernel); 4e-15 is about five times that.
"""
import numpy as np
import pytest

from conftest import golden

import op_ref
from op_ref import CIRC, LIN, SWEEP

REF_TOL = 4e-15


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("BSGP_PERWAVE_MIN_WG", "BSGP_PERWAVE_TW", "BSGP_COOP_ELEMS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c.id)
def test_reference_matches_numpy_operator(case):
    psf, x = case.psf(), case.images()[:2]  # (the third image is zero)
    for tr in (False, True):
        ref = op_ref.op_ref(x, psf, case.mode, tr)
        got = op_ref.numpy_op(x, psf, case.mode, tr)
        for i in (0, 1):
            l2, mx = op_ref.errors(got[i], ref[i])
            print(f"{case.id} {'AT' if tr else 'A'} image {i}: L2 {l2:.2e} max {mx:.2e}")
            assert l2 <= REF_TOL and mx <= REF_TOL, (tr, i, l2, mx)


def test_reference_matches_golden_linear():
    """astropy's convolve_fft (the reference project's A / AT), as recorded."""
    fx = golden("ref_linear_conv.npz")
    for i in range(int(fx["n"])):
        x, k = fx[f"x{i}"], fx[f"k{i}"]
        for name, tr in (("A", False), ("AT", True)):
            l2, mx = op_ref.errors(fx[f"{name}{i}"], op_ref.lin_ref(x, k, tr))
            assert l2 <= REF_TOL and mx <= REF_TOL, (i, name, l2, mx)


def test_known_values():
    """The conventions on inputs small enough to state: fftshift puts the
    centre of an odd PSF at n - 1 (test_odd_circular_operator_fftshift_quirk);
    the linear kernel is centred at k // 2 and AT transposes, not flips."""
    psf = np.zeros((5, 7))
    psf[2, 3] = 1.0
    x = np.zeros((5, 7))
    x[1, 2] = 1.0
    a = np.asarray(op_ref.circ_ref(x, psf), np.float64)
    at = np.asarray(op_ref.circ_ref(x, psf, True), np.float64)
    assert a[0, 1] == 1.0 and a.sum() == 1.0
    assert at[2, 3] == 1.0 and at.sum() == 1.0
    k = np.zeros((2, 3))
    k[0, 2] = 2.0  # normalised to 1: shifts by (0 - 1, 2 - 1)
    x = np.zeros((4, 4))
    x[2, 1] = 3.0
    a = np.asarray(op_ref.lin_ref(x, k), np.float64)
    assert a[1, 2] == 3.0 and a.sum() == 3.0
    # k.T is 3 x 2 with its tap at (2, 0): shifts by (2 - 1, 0 - 1)
    at = np.asarray(op_ref.lin_ref(x, k, True), np.float64)
    assert at[3, 0] == 3.0 and at.sum() == 3.0
    # a leading batch axis; a zero image has no term: exactly zero
    xb = np.stack([x, 2 * x, 0 * x])
    ab = np.asarray(op_ref.lin_ref(xb, k), np.float64)
    assert (ab[0] == a).all() and (ab[1] == 2 * a).all() and not ab[2].any()
    assert not np.asarray(op_ref.circ_ref(np.zeros((2, 5, 7)), psf)).any()


@pytest.mark.skipif(not op_ref.EXTENDED, reason="np.longdouble is float64: one form only")
@pytest.mark.parametrize("cid", ["7x11-circ", "62x93-circ", "33x31-lin-k6x8", "5x7-lin-k9x4",
                                 "40x36-lin-k31x31"])
def test_both_forms_agree(cid):
    """The extended and the double-double form are within the extended form's
    bound of each other: 3 * 2**-64 of sum|terms| (= the value: nothing here
    is negative) per pixel."""
    case = op_ref.BY_ID[cid]
    psf, x = case.psf(), case.images()
    f = op_ref.lin_ref if case.mode == LIN else op_ref.circ_ref
    for tr in (False, True):
        e, d = f(x, psf, tr, extended=True), f(x, psf, tr, extended=False)
        diff = (d.hi.astype(op_ref.LD) - e.hi) + d.lo.astype(op_ref.LD) - e.lo
        assert (np.abs(diff) <= 3 * 2.0 ** -64 * np.abs(np.asarray(e))).all()


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c.id)
def test_sweep_inputs(case):
    psf, x = case.psf(), case.images()
    assert psf.shape == case.kshape and abs(psf.sum() - 1) < 1e-14 and (psf >= 0).all()
    assert psf[0, 0] > 0 and psf[-1, -1] > 0
    if case.mode == CIRC:
        assert np.count_nonzero(psf) <= 40
    assert x.shape == (3, case.H, case.W)
    assert x[0, -1, -1] == 80.0 and (x[0, 0, 0] == 50.0 or case.H * case.W == 1)
    assert not x[1, :-1, :-1].any() and x[1, -1].all() and x[1, :, -1].all()
    assert not x[2].any()


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c.id)
def test_sweep_row_lands_in_its_branch(case):
    assert case.pin, "a row without a purpose"
    assert op_ref.misplaced(case) == {}


def test_sweep_covers_every_regime():
    seen = set()
    for c in SWEEP:
        g = c.layout()
        seen.add((g["coop"], g["nfw"], g["wg_per_cu"]))
    assert {(0, 4, 4), (0, 4, 3), (0, 4, 2), (1, 4, 2), (1, 2, 4), (1, 2, 1), (1, 1, 1)} <= seen
