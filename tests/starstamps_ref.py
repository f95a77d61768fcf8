"""numpy restatements of the two star-stamp kernels, for the
tests: the cutout's box rule with numpy slicing and zero fill, and the score /
strict-minimum / result-row rule built on ``sgp.argmin_strict`` and
``segmentation.shape_columns``."""
import numpy as np

import _bsgp as B
import segmentation
import sgp

BOX_LIMIT = 1 << 30


def box_min(pos, size):
    """astropy 4.3.1 overlap_slices: (int)ceil(pos - size / 2.0) in float64,
    kept inside +-2^30."""
    e = np.ceil(np.float64(pos) - size / 2.0)
    return int(min(max(e, -float(BOX_LIMIT)), float(BOX_LIMIT)))


def cutout_ref(img, positions, size):
    """(stamps, boxes, status) of cutout_stamps: Cutout2D(img, (x, y), size) in
    mode 'trim', the trimmed-away pixels written as 0."""
    img = np.asarray(img)
    H, W = img.shape
    sh, sw = (size, size) if np.ndim(size) == 0 else size
    pos = np.asarray(positions, np.float64).reshape(-1, 2)
    n = len(pos)
    out = np.zeros((n, sh, sw), img.dtype)
    box = np.zeros((n, 4), np.int32)
    st = np.zeros(n, np.int32)
    for i, (x, y) in enumerate(pos):
        if not (np.isfinite(x) and np.isfinite(y)):
            st[i] = B.BSGP_STAMP_BAD_POSITION
            continue
        x0, y0 = box_min(x, sw), box_min(y, sh)
        x1, y1 = x0 + sw, y0 + sh
        box[i] = x0, y0, x1, y1
        if x0 >= W or x1 <= 0 or y0 >= H or y1 <= 0:
            st[i] = B.BSGP_STAMP_NO_OVERLAP
            continue
        xs, xe, ys, ye = max(x0, 0), min(x1, W), max(y0, 0), min(y1, H)
        out[i, ys - y0:ye - y0, xs - x0:xe - x0] = img[ys:ye, xs:xe]
        if (xs, xe, ys, ye) != (x0, x1, y0, y1):
            st[i] = B.BSGP_STAMP_PARTIAL
    return out, box, st


def select_ref(res_nlabels, res_cols, obs_cols, iters, K):
    """(scores, best, rows, num_iters, status) of stamp_select."""
    res_cols, obs_cols = np.asarray(res_cols, np.float64), np.asarray(obs_cols, np.float64)
    n = len(obs_cols)
    scores = np.full((n, K), np.inf)
    best = np.full(n, -1, np.int32)
    rows = np.full((n, B.BSGP_STAMP_ROW_COLS), np.nan)
    nit = np.full(n, -1, np.int32)
    st = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        # shape_columns on whole columns, as the catalogue calls it: numpy's
        # paths for 0-d inputs round about one row in a thousand differently
        sh_o = segmentation.shape_columns(obs_cols[:, 0, 5], obs_cols[:, 0, 6], obs_cols[:, 0, 7])
        sh_r = segmentation.shape_columns(res_cols[:, 0, 5], res_cols[:, 0, 6], res_cols[:, 0, 7])
        for s in range(n):
            o = obs_cols[s, 0]
            sho = {k: v[s] for k, v in sh_o.items()}
            for k in range(K):
                i = s * K + k
                if res_nlabels[i] > 0:
                    scores[s, k] = 1 - res_cols[i, 0, 0] / o[0]
            b = sgp.argmin_strict(scores[s])
            rows[s, 0], rows[s, 5:8] = o[0], (o[3], o[4], sho["fwhm"])
            if K == 1:
                b = 0
                if res_nlabels[s] <= 0:
                    st[s] = B.BSGP_STAMP_RESTORED_NO_SOURCE
            elif b is None:
                st[s] = B.BSGP_STAMP_NO_CANDIDATE
            best[s] = -1 if b is None else b
            if st[s]:
                continue
            r = res_cols[s * K + b, 0]
            shr = {k: v[s * K + b] for k, v in sh_r.items()}
            rows[s, 1:5] = (r[0], 1 - r[0] / o[0], shr["fwhm"] / sho["fwhm"],
                            shr["ellipticity"] / sho["ellipticity"])
            rows[s, 8:11] = r[3], r[4], shr["fwhm"]
            nit[s] = iters[s * K + b]
    return scores, best, rows, nit, st
