"""The per-wave row passes load two adjacent pixels of a row per lane where
that pays (one 16-byte load where there were two of 8 bytes;
bsgp_lanesplit.hpp), keeping every pixel in the accumulator it had before,
and stage a row pair's stored spectrum in 32-byte pieces, so no result bit
may differ from the build before that change.  The fixtures
(tests/golden/make_golden_rowwide.py) are this project's own outputs at that
commit: x (as a SHA-256, and in full for the small float64 cases), discr,
iters and flags, for the phase kernels and the persistent solver, float64 and
float32 storage.  Shapes: one full 64-column chunk; odd H (a last row without
a partner); even W with a partial second chunk (clamped pairs); a chunk
holding a single pair; odd W (the one-pixel path, untouched); the timed
256 x 256 size, alone and as a team of 8.  MI355X tests.
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import make_golden_rowwide as mk  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sgpmod():
    import _bsgp
    _bsgp.require_gpu()
    import sgp
    return sgp


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("persistent", [0, 1])
@pytest.mark.parametrize("name", list(mk.CASES))
def test_bits_of_the_one_pixel_build(sgpmod, name, persistent, storage):
    fx = golden(f"ref_rowwide_{name}.npz")
    gns, _ = mk.inputs(name)
    assert mk.sha(gns) == str(fx["gn_sha"]), "this numpy generates other input images"
    out = mk.solve(sgpmod, name, fx["psf"], persistent, storage)
    k = f"p{persistent}_{storage}_"
    np.testing.assert_array_equal(out["iters"], fx[k + "iters"])
    np.testing.assert_array_equal(out["flags"], fx[k + "flags"])
    np.testing.assert_array_equal(out["discr"], fx[k + "discr"])
    if k + "x" in fx:
        np.testing.assert_array_equal(out["x"], fx[k + "x"])
    assert mk.sha(out["x"]) == str(fx[k + "x_sha"])
