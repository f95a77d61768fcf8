"""``astropy.convolution.convolve`` on the device, for kernels the size of a PSF.

The reference's forward model ``utils.degrade(image, psf)``
(restoration/utils.py:46-56) is ``convolve(image, psf, normalize_kernel=True,
normalization_zero_tol=1e-4)`` with the PSF itself as the kernel, and
``utils.scale_psf(psf, gaussian_fwhm=1.2, size=None)`` (:249-272, used by
``sgp.py --scale_psf``) convolves the PSF with a Gaussian kernel of the PSF's
own size and renormalises.  Both are here under their names, over
``bsgp_convolve2d_ex`` (include/bsgp.h; the rule list is DESIGN §3.12):
astropy's direct sum, bit-defined, for odd kernels up to 63 x 63, with
``boundary='fill'`` and any fill value, both NaN treatments, a mask,
``preserve_nan`` and ``normalize_kernel``.

``segmentation.convolve`` (kernels up to 7 x 7, finite input only) is what
``source_info`` keeps calling; where both paths exist they give the same bits.
Out of scope: the boundaries ``'extend'``, ``'wrap'`` and ``None``,
``convolve_fft``'s keywords and kernels over 63.
"""
import warnings

import numpy as np

import _bsgp as _B
import segmentation as _sg

MAX_KERNEL = _B.BSGP_CONV_MAX_KERNEL
MAX_NORMALIZATION = 100  # astropy's: a kernel whose sum is below 1 / 100 is not normalised
HAD_NAN, NAN_LEFT = _B.BSGP_CONV_HAD_NAN, _B.BSGP_CONV_NAN_LEFT


class NaNLeftWarning(UserWarning):
    """astropy's "nan_treatment='interpolate', however, NaN values detected
    post convolution": a contiguous region of NaN values larger than the
    kernel (or 'fill' with NaNs the sum itself produced)."""


class ConvolveResult(np.ndarray):
    """The float64 result with ``status``: per image (an int for one image)
    ``HAD_NAN`` the input held a NaN or a masked pixel, ``NAN_LEFT`` the output
    holds a NaN that ``preserve_nan`` did not put there."""
    status = None


def make_2dgaussian_kernel(fwhm, size, mode="oversample", oversample=10):
    """photutils' ``make_2dgaussian_kernel`` with ``size`` an odd int or an odd
    pair ``(ny, nx)``; for an int it is ``segmentation.make_2dgaussian_kernel``
    bit for bit."""
    sz = np.atleast_1d(size)
    if sz.size == 1:
        sz = np.repeat(sz, 2)
    if sz.size != 2 or np.any(sz != sz.astype(int)) or np.any(sz < 1) or np.any(sz.astype(int) % 2 == 0):
        raise ValueError(f"size must be an odd positive int or a pair of them, got {size!r}")
    if not fwhm > 0:
        raise ValueError(f"fwhm must be positive, got {fwhm!r}")
    if mode not in ("oversample", "center"):
        raise ValueError(f"mode must be 'oversample' or 'center', got {mode!r}")
    ny, nx = int(sz[0]), int(sz[1])
    f = int(oversample) if mode == "oversample" else 1
    if f < 1:
        raise ValueError(f"oversample must be >= 1, got {oversample!r}")
    sigma = fwhm * _sg.FWHM_TO_SIGMA

    def axis(n):
        lo, hi = -(n // 2), n // 2 + 1
        return np.linspace(lo - 0.5 * (1 - 1 / f), hi - 0.5 * (1 + 1 / f), num=int((hi - lo) * f))

    xg, yg = np.meshgrid(axis(nx), axis(ny))
    # astropy's Gaussian2D.evaluate at theta = 0, operation for operation
    a = 0.5 * (1.0 / sigma ** 2 + 0.0 / sigma ** 2)
    v = 1.0 / (2 * np.pi * sigma * sigma) * np.exp(-((a * xg ** 2) + (0.0 * xg * yg) + (a * yg ** 2)))
    v = v.reshape(ny, f, nx, f).mean(axis=3).mean(axis=1)
    return v / v.sum()


def _host(a):
    torch = _B.torch
    return a.detach().cpu().numpy() if torch is not None and torch.is_tensor(a) else np.asarray(a)


def check_convolve_args(shape, kernel, boundary="fill", fill_value=0.0, nan_treatment="interpolate",
                        normalize_kernel=True, mask_shape=None, normalization_zero_tol=1e-8):
    """The argument checks of :func:`convolve` (host only).  Returns the
    contiguous float64 kernel, ``[kh, kw]`` or ``[B, kh, kw]``, and numpy's
    sum of each kernel (float64 ``[1]`` or ``[B]``)."""
    _sg._check_image_shape(shape, "array")
    if boundary != "fill":
        raise ValueError(f"boundary={boundary!r} is out of scope: only boundary='fill' is offered")
    if nan_treatment not in ("interpolate", "fill"):
        raise ValueError(f"nan_treatment must be 'interpolate' or 'fill', got {nan_treatment!r}")
    try:
        fv = float(fill_value)
    except (TypeError, ValueError):
        fv = np.nan
    if not np.isfinite(fv):
        raise ValueError(f"fill_value must be a finite number, got {fill_value!r}")
    k = np.ascontiguousarray(_host(kernel), dtype=np.float64)
    nb = shape[0] if len(shape) == 3 else 1
    if k.ndim not in (2, 3) or (k.ndim == 3 and (len(shape) != 3 or k.shape[0] != nb)):
        raise ValueError(f"kernel must be [kh, kw], or [B, kh, kw] for a batch of B images, got "
                         f"shape {k.shape} for an array of shape {tuple(shape)}")
    kh, kw = k.shape[-2:]
    if kh % 2 == 0 or kw % 2 == 0 or kh > MAX_KERNEL or kw > MAX_KERNEL:
        raise ValueError(f"kernel of {kh} x {kw}: kernels are odd and at most "
                         f"{MAX_KERNEL} x {MAX_KERNEL}")
    if not np.all(np.isfinite(k)):
        raise ValueError("kernel must be finite")
    if mask_shape is not None and tuple(mask_shape) != tuple(shape):
        raise ValueError(f"mask shape {tuple(mask_shape)} does not match array shape {tuple(shape)}")
    sums = np.array([kk.sum() for kk in (k if k.ndim == 3 else k[None])], dtype=np.float64)
    if normalize_kernel:
        for s in sums:  # astropy's test
            if s < 1.0 / MAX_NORMALIZATION or np.isclose(s, 0, atol=normalization_zero_tol):
                raise ValueError("the kernel can't be normalized, because its sum is close to "
                                 f"zero: the sum of the given kernel is < {1.0 / MAX_NORMALIZATION}")
    return k, sums


def convolve(array, kernel, boundary="fill", fill_value=0.0, nan_treatment="interpolate",
             normalize_kernel=True, mask=None, preserve_nan=False, normalization_zero_tol=1e-8,
             device_out=False):
    """``astropy.convolution.convolve`` with ``boundary='fill'``.

    ``array``: ``[H, W]`` or ``[B, H, W]``, numpy or CUDA tensor, float32 or
    float64 (anything else is converted to float64); the result is float64 of
    the same shape.  ``kernel``: odd ``[kh, kw]`` up to 63 x 63, or
    ``[B, kh, kw]``, image b with kernel b.  ``mask``: nonzero = masked, of
    ``array``'s shape.  An image that holds a NaN or masked pixel is
    interpolated as a whole (``nan_treatment='interpolate'``, astropy's
    default) or has those pixels replaced by ``fill_value`` (``'fill'``).

    Returns a :class:`ConvolveResult` (numpy, with ``status``), or with
    ``device_out`` the pair (CUDA tensor, int32 status tensor ``[B]``) without
    waiting for the device.  A NaN left in the output raises a
    :class:`NaNLeftWarning` (not with ``device_out``: look at the status)."""
    shape = _sg._shape_of(array)
    k, sums = check_convolve_args(shape, kernel, boundary, fill_value, nan_treatment,
                                  normalize_kernel, None if mask is None else _sg._shape_of(mask),
                                  normalization_zero_tol)
    _B.require_gpu()
    torch = _B.torch
    d, batched = _sg._to_dev(array)
    B, H, W = d.shape
    kd, sd = torch.from_numpy(k).to("cuda"), torch.from_numpy(sums).to("cuda")
    md = None
    if mask is not None:
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(_host(mask) != 0))
        md = (m != 0).to(device="cuda", dtype=torch.uint8).reshape(B, H, W).contiguous()
    flags = (_B.BSGP_CONV_F_FILL if nan_treatment == "fill" else _B.BSGP_CONV_F_INTERPOLATE) \
        | (_B.BSGP_CONV_F_NORMALIZE if normalize_kernel else 0) \
        | (_B.BSGP_CONV_F_PRESERVE_NAN if preserve_nan else 0)
    out = torch.empty((B, H, W), dtype=torch.float64, device="cuda")
    status = torch.empty((B,), dtype=torch.int32, device="cuda")
    kh, kw = k.shape[-2:]
    _B.check(_B.lib().bsgp_convolve2d_ex(_B._ptr(d), _sg._dtype(d), B, H, W, _B._ptr(kd), kh, kw,
                                         kh * kw if k.ndim == 3 else 0, _B._ptr(sd), _B._ptr(md),
                                         flags, float(fill_value), _B._ptr(out), _B._ptr(status),
                                         _B.current_stream()))
    out._keep = (d, kd, sd, md)
    if device_out:
        return (out if batched else out[0]), status
    st = status.cpu().numpy()
    res = (out if batched else out[0]).cpu().numpy().view(ConvolveResult)
    res.status = st if batched else int(st[0])
    if np.any(st & NAN_LEFT):
        warnings.warn("NaN values detected post convolution: a contiguous region of NaN values, "
                      "larger than the kernel size, is present in the input array (or the sum "
                      "itself produced one). Increase the kernel size to avoid this.",
                      NaNLeftWarning, stacklevel=2)
    return res


def degrade(image, psf, device_out=False):
    """The reference's forward model (restoration/utils.py:46-56):
    ``convolve(image, psf, normalize_kernel=True, normalization_zero_tol=1e-4)``.
    ``image`` may be a batch and ``psf`` one stamp per image."""
    return convolve(image, psf, normalize_kernel=True, normalization_zero_tol=1e-4,
                    device_out=device_out)


def scale_psf(psf, gaussian_fwhm=1.2, size=None, device_out=False):
    """The reference's ``scale_psf`` (restoration/utils.py:249-272): the PSF
    convolved with ``make_2dgaussian_kernel(gaussian_fwhm, size)`` (``size``
    defaults to the stamp's ``(ny, nx)``), divided by its sum.  ``psf``: one
    stamp or ``[n, S, S]``; every stamp is divided by its own sum, summed on
    the device in a fixed order."""
    shape = _sg._shape_of(psf)
    _sg._check_image_shape(shape, "psf")
    kernel = make_2dgaussian_kernel(gaussian_fwhm, tuple(shape[-2:]) if size is None else size)
    conv, status = convolve(psf, kernel, device_out=True)
    out = conv / conv.sum(dim=(-2, -1), keepdim=True)
    if device_out:
        return out
    if np.any(status.cpu().numpy() & NAN_LEFT):
        warnings.warn("NaN values detected post convolution", NaNLeftWarning, stacklevel=2)
    return out.cpu().numpy()
