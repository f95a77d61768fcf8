"""numpy restatement of the source validation, for
the tests: the three zero-filled windows by numpy slicing with the cutouts'
box rule (``starstamps_ref.box_min``), then ``np.sort(...)[-3:].mean()``,
``np.median`` and ``np.mean`` of contiguous arrays, and the strict float64
comparison.  Written from the rule, not from the reference's code."""
import warnings

import numpy as np

import _bsgp as B
from starstamps_ref import box_min


def _size(size):
    return (int(size), int(size)) if np.ndim(size) == 0 else (int(size[0]), int(size[1]))


def window(frame, x0, y0, sh, sw):
    """V1: the sh x sw cells from (y0, x0), 0.0 outside the frame, contiguous,
    in the frame's dtype."""
    H, W = frame.shape
    out = np.zeros((sh, sw), frame.dtype)
    xs, xe, ys, ye = max(x0, 0), min(x0 + sw, W), max(y0, 0), min(y0 + sh, H)
    if xs < xe and ys < ye:
        out[ys - y0:ye - y0, xs - x0:xe - x0] = frame[ys:ye, xs:xe]
    return out


def validate_one(image, coord, bkgmap, rmsmap, size=100, nsigma=3.0):
    """(valid, source_pixs, bkg, rms, status) of one source at coord = (x, y)."""
    image = np.asarray(image)
    bkgmap, rmsmap = np.asarray(bkgmap, np.float64), np.asarray(rmsmap, np.float64)
    H, W = image.shape
    sh, sw = _size(size)
    x, y = float(coord[0]), float(coord[1])
    nan = float("nan")
    if not (np.isfinite(x) and np.isfinite(y)):  # V6
        return False, nan, nan, nan, B.BSGP_STAMP_BAD_POSITION
    x0, y0 = box_min(x, sw), box_min(y, sh)
    if x0 >= W or x0 + sw <= 0 or y0 >= H or y0 + sh <= 0:
        return False, nan, nan, nan, B.BSGP_STAMP_NO_OVERLAP
    st = B.BSGP_STAMP_PARTIAL if (x0 < 0 or y0 < 0 or x0 + sw > W or y0 + sh > H) else 0
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        c = window(image, x0, y0, sh, sw)
        source_pixs = np.sort(c.flatten())[-3:].mean()  # V2, in the image's dtype
        bkg = np.median(window(bkgmap, x0, y0, sh, sw))  # V3
        rms = np.mean(window(rmsmap, x0, y0, sh, sw))  # V4: contiguous, numpy's pairwise sum
        valid = bool(np.float64(source_pixs) > np.float64(bkg) + np.float64(nsigma) * np.float64(rms))
    return valid, float(source_pixs), float(bkg), float(rms), st


def validate_ref(image, positions, bkgmap, rmsmap, size=100, nsigma=3.0):
    """dict of arrays over the positions [n, 2]: valid (bool), stats [n, 3] =
    source_pixs, bkg, rms, status (int32)."""
    pos = np.asarray(positions, np.float64).reshape(-1, 2)
    rows = [validate_one(image, p, bkgmap, rmsmap, size, nsigma) for p in pos]
    return dict(valid=np.array([r[0] for r in rows], bool),
                stats=np.array([r[1:4] for r in rows], np.float64).reshape(-1, 3),
                status=np.array([r[4] for r in rows], np.int32))
