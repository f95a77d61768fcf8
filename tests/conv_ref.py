"""Plain-numpy restatement of DESIGN §3.12: astropy.convolution.convolve with
boundary='fill' for kernels of any odd size.  It is seg_ref.convolve (taps in
row-major order of the window, tap (i, j) times K[kh-1-i][kw-1-j], every
product and sum rounded, one division) plus the fill value, the mask, both NaN
treatments, preserve_nan and normalize_kernel.  tests/golden/ref_linear_conv.npz
pins it to astropy (tests/test_convolution.py)."""
import numpy as np

import seg_ref  # noqa: F401  (the NaN-free case must equal seg_ref.convolve bit for bit)

HAD_NAN, NAN_LEFT = 1, 2


def convolve(data, kernel, fill_value=0.0, nan_treatment="interpolate", normalize_kernel=True,
             mask=None, preserve_nan=False, return_status=False):
    """One image [H, W]; returns the float64 result (and the status bits)."""
    d = np.array(data).astype(np.float64)
    k = np.asarray(kernel, dtype=np.float64)
    kh, kw = k.shape
    H, W = d.shape
    if mask is not None:
        d[np.asarray(mask) != 0] = np.nan
    was_nan = np.isnan(d)
    had = bool(was_nan.any())
    centre = d.copy()
    if nan_treatment == "fill":
        d[was_nan] = fill_value
    interp = had and nan_treatment == "interpolate"
    ksum = k.sum()
    P = np.full((H + kh - 1, W + kw - 1), float(fill_value))
    P[kh // 2:kh // 2 + H, kw // 2:kw // 2 + W] = d
    top, bot = np.zeros((H, W)), np.zeros((H, W))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(kh):
            for j in range(kw):
                v, kk = P[i:i + H, j:j + W], k[kh - 1 - i, kw - 1 - j]
                if interp:
                    ok = ~np.isnan(v)
                    top = np.where(ok, top + v * kk, top)
                    bot = np.where(ok, bot + kk, bot)
                else:
                    top = top + v * kk
        if interp:
            out = np.where(bot == 0, centre, top / bot)
            if not normalize_kernel:
                out = out * ksum
        else:
            out = top / ksum if normalize_kernel else top
    if preserve_nan:
        out[was_nan] = np.nan
    left = np.isnan(out) & ~(was_nan if preserve_nan else np.zeros_like(was_nan))
    status = (HAD_NAN if had else 0) | (NAN_LEFT if left.any() else 0)
    return (out, status) if return_status else out


def convolve_batch(data, kernel, mask=None, **kw):
    """[B, H, W] with one kernel or [B, kh, kw]: (results, status array)."""
    k = np.asarray(kernel)
    res = [convolve(data[b], k[b] if k.ndim == 3 else k, mask=None if mask is None else mask[b],
                    return_status=True, **kw) for b in range(len(data))]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32)
