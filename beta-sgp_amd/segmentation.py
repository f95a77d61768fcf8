"""Source detection and segment fluxes on the device.

The reference's ``utils.source_info`` (restoration/utils.py:219-247) runs
photutils: ``Background2D``, ``convolve`` with ``make_2dgaussian_kernel(1.2, 3)``,
``SourceFinder(npixels, ...)`` and ``SourceCatalog``.  The application uses its
result for the flux constraint of every solve,
``flux=orig_scat['segment_flux'].value.sum()``
(application_sgp_subdivisions.py:88,104,113), and for the score that ranks the
beta candidates, ``1 - sum(segment_flux(restored)) / sum(segment_flux(original))``
(:92-99).  This module computes both with ``bsgp_convolve2d``,
``bsgp_detect_sources`` and ``bsgp_segment_catalog`` (include/bsgp.h; semantics
in DESIGN §3.8) and keeps photutils' names.

What is pinned and what is not: the kernel equals astropy's at rtol 1e-13, the
convolution equals astropy's to the last bit, the label image equals ``scipy.ndimage.label`` followed by the
removal of small components and a consecutive relabel, which is photutils'
``detect_sources``.  Deblending (``SourceFinder(deblend=True)``,
:func:`deblend_sources`, ``bsgp_deblend_sources``) is modelled on photutils'
documented ``deblend_sources`` and pinned to the parts it is built from,
``scipy.ndimage.label`` and ``skimage.segmentation.watershed`` (DESIGN §3.8,
steps D1 to D7).  It splits a segment among children without dropping a pixel,
so at ``localbkg_width=0`` the sum of ``segment_flux`` over all segments is
the same with and without it; ``source_info`` therefore deblends only on
request (``deblend=True``).  The moment and shape columns are defined in
DESIGN §3.8, modelled on photutils' documentation but not pinned to it.

The reference builds its catalogue with ``SourceCatalog(...,
localbkg_width=5)`` (utils.py:244-246): photutils measures a local background
in a rectangular annulus around every source and subtracts it from
``segment_flux``, ``min_value`` and ``max_value``.  ``localbkg_width > 0`` does
the same here (``bsgp_segment_local_background``, DESIGN §3.8 L1 to L6,
modelled on photutils and pinned to the catalogue the reference published for
its frame).  Then every segment has its own box, annulus and area, so the sum
over segments depends on the deblending: the reference's flux constraint is
``localbkg_width=5`` together with ``deblend=True``.  The default is 0
everywhere, which leaves the columns as they were.
"""
import ctypes
import warnings

import numpy as np

import _bsgp as _B

FWHM_TO_SIGMA = 1.0 / (2.0 * np.sqrt(2.0 * np.log(2.0)))
MAX_KERNEL = 7

INT_COLUMNS = ("area", "bbox_xmin", "bbox_xmax", "bbox_ymin", "bbox_ymax")
F64_COLUMNS = ("segment_flux", "min_value", "max_value", "xcentroid", "ycentroid",
               "covar_sigx2", "covar_sigxy", "covar_sigy2")
SHAPE_COLUMNS = ("semimajor_sigma", "semiminor_sigma", "orientation", "eccentricity",
                 "ellipticity", "fwhm")
COLUMNS = ("label",) + INT_COLUMNS + F64_COLUMNS + SHAPE_COLUMNS
UNAVAILABLE = {
    "sky_centroid": "there is no WCS here: use xcentroid / ycentroid",
    "local_background": "no local background was measured: pass localbkg_width > 0 "
                        "(photutils' localbkg_width; the reference uses 5)",
    "segment_fluxerr": "no error array is carried: photometric errors are out of scope",
}


class NoDetectionsWarning(UserWarning):
    """No source was found (photutils' warning of the same name)."""


class DeblendBoxWarning(UserWarning):
    """A parent segment's bounding box holds more than DEBLEND_MAX_BOX pixels
    (with ``large_parents=True``: the segment holds more than
    DEBLEND_LARGE_MAX_AREA pixels): it is left undeblended."""


class LocalBackgroundCapWarning(UserWarning):
    """The local-background annulus of a source holds more than LOCALBKG_MAX
    values: its local background is 0 and its columns are left uncorrected."""


DEBLEND_MAX_BOX = _B.BSGP_DEBLEND_MAX_BOX
LOCALBKG_MAX = _B.BSGP_LOCALBKG_MAX
LOCALBKG_SIGMA, LOCALBKG_MAXITERS, LOCALBKG_MIN_PIXELS = 3.0, 10, 10  # photutils' constants
DEBLEND_LARGE_MAX_AREA = _B.BSGP_DEBLEND_LARGE_MAX_AREA
DEBLEND_MODES = {"linear": _B.BSGP_DEBLEND_LINEAR, "exponential": _B.BSGP_DEBLEND_EXPONENTIAL}


def make_2dgaussian_kernel(fwhm, size, mode="oversample", oversample=10):
    """photutils' ``make_2dgaussian_kernel``: astropy's
    ``Gaussian2DKernel(fwhm * gaussian_fwhm_to_sigma, x_size=size, y_size=size,
    mode='oversample', factor=oversample)``, normalised to sum 1 (host, numpy).
    Every pixel is the mean of the Gaussian over oversample x oversample
    sub-pixel centres; ``mode='center'`` samples the pixel centres."""
    if int(size) != size or size < 1 or int(size) % 2 == 0:
        raise ValueError(f"size must be an odd positive int, got {size!r}")
    if not fwhm > 0:
        raise ValueError(f"fwhm must be positive, got {fwhm!r}")
    if mode not in ("oversample", "center"):
        raise ValueError(f"mode must be 'oversample' or 'center', got {mode!r}")
    size = int(size)
    f = int(oversample) if mode == "oversample" else 1
    if f < 1:
        raise ValueError(f"oversample must be >= 1, got {oversample!r}")
    sigma = fwhm * FWHM_TO_SIGMA
    lo, hi = -(size // 2), size // 2 + 1
    x = np.linspace(lo - 0.5 * (1 - 1 / f), hi - 0.5 * (1 + 1 / f), num=int((hi - lo) * f))
    xg, yg = np.meshgrid(x, x)
    # astropy's Gaussian2D.evaluate at theta = 0, operation for operation
    a = 0.5 * (1.0 / sigma ** 2 + 0.0 / sigma ** 2)
    v = 1.0 / (2 * np.pi * sigma * sigma) * np.exp(-((a * xg ** 2) + (0.0 * xg * yg) + (a * yg ** 2)))
    v = v.reshape(size, f, size, f).mean(axis=3).mean(axis=1)
    return v / v.sum()


def _check_kernel(kernel):
    k = np.asarray(kernel, dtype=np.float64)
    if k.ndim != 2:
        raise ValueError(f"kernel must be 2-D, got shape {k.shape}")
    kh, kw = k.shape
    if kh % 2 == 0 or kw % 2 == 0 or kh > MAX_KERNEL or kw > MAX_KERNEL:
        raise ValueError(f"kernel of {kh} x {kw}: kernels are odd and at most "
                         f"{MAX_KERNEL} x {MAX_KERNEL}")
    if not np.all(np.isfinite(k)) or k.sum() == 0:
        raise ValueError("kernel must be finite with a nonzero sum")
    return np.ascontiguousarray(k)


def _shape_of(a):
    torch = _B.torch
    return tuple(a.shape) if torch is not None and torch.is_tensor(a) else np.shape(a)


def _check_image_shape(shape, name="data"):
    if len(shape) not in (2, 3) or 0 in shape:
        raise ValueError(f"{name} must be [H, W] or [B, H, W], got shape {tuple(shape)}")


def _to_dev(data, keep_f32=True):
    """float32 / float64 CUDA tensor [B, H, W] and whether data was a batch."""
    torch = _B.torch
    if torch.is_tensor(data):
        ok = (torch.float32, torch.float64) if keep_f32 else (torch.float64,)
        d = data if data.dtype in ok else data.to(torch.float64)
        d = d.to("cuda").contiguous()
    else:
        d = np.asarray(data)
        if not (d.dtype.kind == "f" and d.dtype.itemsize in ((4, 8) if keep_f32 else (8,))):
            d = d.astype(np.float64)
        d = torch.from_numpy(np.ascontiguousarray(d.astype(d.dtype.newbyteorder("=")))).to("cuda")
    batched = d.dim() == 3
    return (d if batched else d[None]), batched


def _dtype(d):
    return _B.BSGP_DTYPE_F32 if d.dtype == _B.torch.float32 else _B.BSGP_DTYPE_F64


def _out(t, batched, device_out):
    t = t if batched else t[0]
    return t if device_out else t.cpu().numpy()


def check_localbkg_width(localbkg_width):
    """The argument check of ``localbkg_width`` (host only): a finite number
    >= 0 (photutils takes an int; any finite width is served)."""
    w = localbkg_width
    if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)) \
            or not np.isfinite(w) or w < 0:
        raise ValueError(f"localbkg_width must be a finite number >= 0, got {localbkg_width!r}")
    return float(w)


def convolve(data, kernel, device_out=False):
    """``astropy.convolution.convolve(data, kernel)`` with its defaults on
    finite input: zero fill, kernel normalised by its sum.  float64 result of
    data's shape.  A non-finite pixel raises ``ValueError`` (astropy's NaN
    interpolation is not offered)."""
    _check_image_shape(_shape_of(data))
    k = _check_kernel(kernel)
    _B.require_gpu()
    torch = _B.torch
    d, batched = _to_dev(data)
    if not bool(torch.isfinite(d).all()):
        raise ValueError("data holds non-finite pixels: NaN interpolation is not offered")
    return _out(_convolve_dev(d, k), batched, device_out)


def _convolve_dev(d, k):
    torch = _B.torch
    B, H, W = d.shape
    kd = torch.from_numpy(k).to("cuda")
    out = torch.empty((B, H, W), dtype=torch.float64, device="cuda")
    _B.check(_B.lib().bsgp_convolve2d(_B._ptr(d), _dtype(d), B, H, W, _B._ptr(kd), k.shape[0],
                                      k.shape[1], _B._ptr(out), _B.current_stream()))
    out._keep = (d, kd)
    return out


class SegmentationImage:
    """Result of :func:`detect_sources`: ``data`` (int32 label image, 0 =
    background), ``nlabels``, ``labels`` (1..nlabels) and ``areas`` (pixels per
    label).  For a batch ``data`` is [B, H, W], ``nlabels`` an int array [B]
    and ``labels`` / ``areas`` lists of B arrays.  The result of
    :func:`deblend_sources` also carries ``parent``, per label the label of the
    input segment it came from, and ``status``, the ``BSGP_DEBLEND_*`` bits the
    device set per image (both ``None`` otherwise)."""

    def __init__(self, data, nlabels, batched, parent=None, status=None):
        self.data, self.batched = data, batched
        self.nlabels = nlabels if batched else int(nlabels[0])
        self._n = np.asarray(nlabels)
        self.parent = parent if parent is None or batched else parent[0]
        self.status = status if status is None or batched else int(status[0])

    @property
    def labels(self):
        out = [np.arange(1, n + 1, dtype=np.int32) for n in self._n]
        return out if self.batched else out[0]

    @property
    def areas(self):
        torch = _B.torch
        lab = self.data if self.batched else self.data[None]
        lab = lab.cpu().numpy() if torch is not None and torch.is_tensor(lab) else np.asarray(lab)
        out = [np.bincount(l.ravel(), minlength=n + 1)[1:] for l, n in zip(lab, self._n)]
        return out if self.batched else out[0]


def check_detect_args(shape, npixels, connectivity, threshold_shape=(), mask_shape=None):
    """The argument checks of detect_sources (host only)."""
    _check_image_shape(shape)
    if int(npixels) != npixels or npixels < 1:
        raise ValueError(f"npixels must be a positive int, got {npixels!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    for nm, s in (("threshold", threshold_shape), ("mask", mask_shape)):
        if s is None or (nm == "threshold" and tuple(s) == ()):
            continue
        if tuple(s) != tuple(shape) and tuple(s) != tuple(shape[-2:]):
            raise ValueError(f"{nm} shape {tuple(s)} does not match data shape {tuple(shape)}")


def detect_sources(data, threshold, npixels, connectivity=8, mask=None, device_out=False):
    """photutils' ``detect_sources``: pixels with ``data > threshold`` (a
    scalar or a map; masked or non-finite pixels never), grouped with 8- or
    4-connectivity, groups of fewer than ``npixels`` pixels removed, the others
    numbered 1..n by their first pixel in raster order.  An unbatched call that
    detects nothing warns and returns ``None``; in a batch such an image has
    ``nlabels == 0``."""
    check_detect_args(_shape_of(data), npixels, connectivity, _shape_of(threshold),
                      None if mask is None else _shape_of(mask))
    _B.require_gpu()
    d, batched = _to_dev(data)
    seg = _detect_dev(d, threshold, int(npixels), int(connectivity), mask)
    lab, n = seg
    if not batched and n[0] == 0:
        warnings.warn("No sources were found.", NoDetectionsWarning)
        return None
    return SegmentationImage(_out(lab, batched, device_out), n, batched)


def _detect_dev(d, threshold, npixels, connectivity, mask):
    """(int32 CUDA labels [B, H, W], host nlabels [B]); one synchronisation."""
    torch = _B.torch
    B, H, W = d.shape
    thr_map, thr = None, 0.0
    if torch.is_tensor(threshold) or np.ndim(threshold) > 0:
        t, _ = _to_dev(threshold, keep_f32=False)
        thr_map = t.expand(B, H, W).contiguous()
    else:
        thr = float(threshold)
    m = None
    if mask is not None:
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
        m = (m != 0).to("cuda")
        m = (m[None] if m.dim() == 2 else m).expand(B, H, W).to(torch.uint8).contiguous()
    lab = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
    n = torch.empty((B,), dtype=torch.int32, device="cuda")
    _B.check(_B.lib().bsgp_detect_sources(_B._ptr(d), _dtype(d), B, H, W, _B._ptr(thr_map), thr,
                                          npixels, connectivity, _B._ptr(m), _B._ptr(lab),
                                          _B._ptr(n), _B.current_stream()))
    return lab, n.cpu().numpy()  # waits for the kernels (d, thr_map, m are alive until here)


def check_deblend_args(shape, seg_shape, npixels, nlevels=32, contrast=0.001, mode="exponential",
                       connectivity=8, relabel=True, large_parents=False, lds_max_box=None):
    """The argument checks of deblend_sources (host only)."""
    _check_image_shape(shape)
    if tuple(seg_shape) != tuple(shape):
        raise ValueError(f"segment_img shape {tuple(seg_shape)} does not match data shape "
                         f"{tuple(shape)}")
    if int(npixels) != npixels or npixels < 1:
        raise ValueError(f"npixels must be a positive int, got {npixels!r}")
    if int(nlevels) != nlevels or nlevels < 1:
        raise ValueError(f"nlevels must be a positive int, got {nlevels!r}")
    if not 0.0 <= contrast <= 1.0:
        raise ValueError(f"contrast must lie in [0, 1], got {contrast!r}")
    if mode == "sinh":
        raise ValueError("mode 'sinh' is not offered: use 'exponential' or 'linear'")
    if mode not in DEBLEND_MODES:
        raise ValueError(f"mode must be 'exponential' or 'linear', got {mode!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if not relabel:
        raise ValueError("relabel=False is not offered: the output labels are consecutive")
    if not isinstance(large_parents, (bool, np.bool_)):
        raise ValueError(f"large_parents must be a bool, got {large_parents!r}")
    if lds_max_box is None:
        return
    if isinstance(lds_max_box, (bool, np.bool_)) or int(lds_max_box) != lds_max_box \
            or not 0 <= lds_max_box <= DEBLEND_MAX_BOX:
        raise ValueError(f"lds_max_box must be an int in 0..{DEBLEND_MAX_BOX}, got {lds_max_box!r}")
    if not large_parents and lds_max_box != DEBLEND_MAX_BOX:
        raise ValueError("lds_max_box needs large_parents=True: without the global-memory path "
                         f"the LDS cap is {DEBLEND_MAX_BOX}")


def deblend_numbering(nchild, present=None):
    """D7 on the host (the rule k_deblend_number implements): from the number of
    children per input label 1..n (0 = left as it is) the output label of every
    parent left as it is, the first child's label of every split parent, and
    the number of output labels.  ``present``: labels the image holds."""
    nchild = np.asarray(nchild, dtype=np.int64)
    present = np.ones(len(nchild), bool) if present is None else np.asarray(present, bool)
    kept = present & (nchild == 0)
    kids = np.where(present, nchild, 0)
    base = np.zeros(len(nchild), dtype=np.int64)
    base[kept] = np.arange(1, kept.sum() + 1)
    first = kept.sum() + 1 + np.cumsum(kids) - kids
    base[kids > 0] = first[kids > 0]
    return base, int(kept.sum() + kids.sum())


def _deblend_dev(d, lab, n, npixels, nlevels, contrast, mode, connectivity, select=None,
                 large_parents=False, lds_max_box=DEBLEND_MAX_BOX):
    """(int32 CUDA labels [B, H, W], host nlabels [B], host status [B], int32
    CUDA parents [B, max nlabels + 1]) of the deblended image; one wait for the
    kernels.  d: float64 CUDA [B, H, W]; lab: int32 CUDA; n: host
    int32 [B]; select: host bool [B, cap] or None.  large_parents:
    bsgp_deblend_sources_large with lds_max_box, else bsgp_deblend_sources."""
    torch = _B.torch
    B, H, W = d.shape
    n = np.ascontiguousarray(n, dtype=np.int32)
    cap = max(1, int(n.max()))
    nd = torch.from_numpy(n).to("cuda")
    ic = torch.empty((B, cap, 5), dtype=torch.int32, device="cuda")
    fc = torch.empty((B, cap, 8), dtype=torch.float64, device="cuda")
    st = torch.empty((B,), dtype=torch.int32, device="cuda")
    _B.check(_B.lib().bsgp_segment_catalog(_B._ptr(d), None, _B._ptr(lab), B, H, W, cap, _B._ptr(nd),
                                           _B._ptr(ic), _B._ptr(fc), _B._ptr(st),
                                           _B.current_stream()))
    sel = None
    if select is not None:
        sel = torch.from_numpy(np.ascontiguousarray(select, dtype=np.uint8)).to("cuda")
    out = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
    nout = torch.empty((B,), dtype=torch.int32, device="cuda")
    dst = torch.empty((B,), dtype=torch.int32, device="cuda")
    head = (_B._ptr(d), _B._ptr(lab), B, H, W, cap, _B._ptr(nd), _B._ptr(ic), _B._ptr(sel),
            int(npixels), int(nlevels), float(contrast), DEBLEND_MODES[mode], int(connectivity))
    tail = (_B._ptr(out), _B._ptr(nout), _B._ptr(dst), _B.current_stream())
    if large_parents:
        _B.check(_B.lib().bsgp_deblend_sources_large(*head, int(lds_max_box), *tail))
    else:
        _B.check(_B.lib().bsgp_deblend_sources(*head, *tail))
    # the count for the warning, by the kernel's own rule; which images hold such a parent is
    # the kernel's status bit, and the two must agree
    box = (ic[..., 2] - ic[..., 1] + 1).long() * (ic[..., 4] - ic[..., 3] + 1).long()
    if large_parents:  # the area rule of the global-memory path
        over = (box > int(lds_max_box)) & (ic[..., 0] > DEBLEND_LARGE_MAX_AREA)
    else:
        over = box > DEBLEND_MAX_BOX
    over &= ic[..., 0] >= 2 * int(npixels)
    over &= torch.arange(cap, device="cuda")[None, :] < nd[:, None]
    if sel is not None:
        over &= sel != 0
    host = torch.stack([nout, dst, st, over.sum(dim=1).to(torch.int32)]).cpu().numpy()
    nout_h, status, cat_status, nover = host[0].astype(np.int32), host[1], host[2], host[3]
    if cat_status.any() or (status & _B.BSGP_DEBLEND_BAD_LABEL).any():
        bad = np.flatnonzero(cat_status | (status & _B.BSGP_DEBLEND_BAD_LABEL))
        raise _B.BsgpError(_B.BSGP_ERR_ARG, f"image {int(bad[0])}: labels outside 1..nlabels in "
                           "the segmentation image")
    flagged = (status & _B.BSGP_DEBLEND_OVER_CAP) != 0
    if not np.array_equal(flagged, nover > 0):
        raise _B.BsgpError(_B.BSGP_ERR_HIP, "bsgp_deblend_sources reports parents over the cap "
                           f"in images {np.flatnonzero(flagged).tolist()}, int_cols hold them in "
                           f"images {np.flatnonzero(nover > 0).tolist()}")
    if flagged.any():
        what = (f"of more than {DEBLEND_LARGE_MAX_AREA} pixels (the area limit of large_parents)"
                if large_parents else f"with a bounding box of more than {DEBLEND_MAX_BOX} pixels")
        warnings.warn(f"{int(nover[flagged].sum())} parent segment(s) {what} were left "
                      "undeblended", DeblendBoxWarning)
    # parent of every output label: every pixel of a label writes the same input label
    par = torch.zeros((B, int(nout_h.max()) + 1), dtype=torch.int32, device="cuda")
    par.scatter_(1, out.reshape(B, -1).long(), lab.reshape(B, -1))
    return out, nout_h, status.astype(np.int32), par


def _deblended_image(res, batched, device_out):
    """The SegmentationImage of _deblend_dev's result."""
    out, n, status, par = res
    par = par if device_out else par.cpu().numpy()
    return SegmentationImage(_out(out, batched, device_out), n, batched,
                             parent=[par[b, 1:k + 1] for b, k in enumerate(n)], status=status)


def _labels_dev(segment_img, batched):
    """(int32 CUDA labels [B, H, W], host nlabels [B]) of a SegmentationImage or
    a label image."""
    torch = _B.torch
    seg = segment_img.data if isinstance(segment_img, SegmentationImage) else segment_img
    lab = seg if torch.is_tensor(seg) else torch.from_numpy(np.ascontiguousarray(seg))
    lab = lab.to(device="cuda", dtype=torch.int32).contiguous()
    lab = lab if batched else lab[None]
    if isinstance(segment_img, SegmentationImage):
        return lab, np.asarray(segment_img._n, dtype=np.int32)
    if bool((lab < 0).any()):
        raise ValueError("segment_img holds negative labels")
    return lab, lab.reshape(lab.shape[0], -1).amax(dim=1).cpu().numpy().astype(np.int32)


def deblend_sources(data, segment_img, npixels, labels=None, nlevels=32, contrast=0.001,
                    mode="exponential", connectivity=8, relabel=True, device_out=False,
                    large_parents=False, lds_max_box=DEBLEND_MAX_BOX):
    """photutils' ``deblend_sources`` for an image or a batch: every segment of
    ``segment_img`` (a :class:`SegmentationImage` or an integer label image) is
    split by multi-thresholding (``nlevels`` levels between its minimum and
    maximum of ``data``, spaced by ``mode`` 'exponential' or 'linear';
    components of at least ``npixels`` pixels) and a watershed, and children
    below ``contrast`` of the segment's flux are merged back (DESIGN §3.8, D1
    to D7).  ``data`` is the image the segments were detected in (the
    convolved one in ``source_info``).  ``labels``: deblend only these labels
    (of every image of a batch that holds them; 1..max ``nlabels``).  Returns a :class:`SegmentationImage` with
    consecutive labels -- the segments left as they are first, in their order,
    then the children by parent -- that also carries ``parent`` and ``status``
    (CUDA tensors with ``device_out=True``).  A segment
    whose bounding box holds more than ``DEBLEND_MAX_BOX`` pixels is left as it
    is, with one :class:`DeblendBoxWarning` per call.  With
    ``large_parents=True`` (``bsgp_deblend_sources_large``) such a segment is
    deblended too, by the kernel that works in global memory, and gets the
    labels the LDS kernel would give it; only a segment of more than
    ``DEBLEND_LARGE_MAX_AREA`` pixels is left, flagged and warned about.
    ``lds_max_box`` (0..``DEBLEND_MAX_BOX``, with ``large_parents=True`` only)
    moves the border between the two kernels; 0 sends every segment through
    the global-memory one.  ``mode='sinh'`` and ``relabel=False`` raise
    ``ValueError``."""
    seg = segment_img.data if isinstance(segment_img, SegmentationImage) else segment_img
    check_deblend_args(_shape_of(data), _shape_of(seg), npixels, nlevels, contrast, mode,
                       connectivity, relabel, large_parents, lds_max_box)
    _B.require_gpu()
    d, batched = _to_dev(data, keep_f32=False)
    lab, n = _labels_dev(segment_img, batched)
    select = None
    if labels is not None:
        want = np.atleast_1d(np.asarray(labels)).astype(np.int64)
        top = int(n.max()) if batched else int(n[0])
        if want.size and (want.min() < 1 or want.max() > top):
            raise ValueError(f"labels must lie in 1..{top}, got {labels!r}")
        select = np.zeros((d.shape[0], max(1, int(n.max()))), dtype=bool)
        select[:, want - 1] = True  # an image of a batch without such a label has no such row
    res = _deblend_dev(d, lab, n, npixels, nlevels, contrast, mode, connectivity, select,
                       bool(large_parents), int(lds_max_box))
    return _deblended_image(res, batched, device_out)


class SourceFinder:
    """photutils' ``SourceFinder(npixels, connectivity=8, deblend=True, nlevels=32,
    contrast=0.001, mode='exponential')`` as ``utils.source_info`` builds it
    (restoration/utils.py:235): ``finder(data, threshold, mask=None)`` is
    :func:`detect_sources` followed, when ``deblend``, by
    :func:`deblend_sources`.  ``relabel``, ``nproc`` and ``progress_bar`` are
    accepted for the signature; ``nproc`` and ``progress_bar`` are ignored.
    ``large_parents`` as in :func:`deblend_sources`."""

    def __init__(self, npixels, connectivity=8, deblend=True, nlevels=32, contrast=0.001,
                 mode="exponential", relabel=True, nproc=1, progress_bar=True, device_out=False,
                 large_parents=False):
        check_detect_args((1, 1), npixels, connectivity)
        check_deblend_args((1, 1), (1, 1), npixels, nlevels, contrast, mode, connectivity, relabel,
                           large_parents)
        self.large_parents = bool(large_parents)
        self.npixels, self.connectivity, self.deblend = int(npixels), int(connectivity), bool(deblend)
        self.nlevels, self.contrast, self.mode = int(nlevels), float(contrast), mode
        self.device_out = device_out

    def __call__(self, data, threshold, mask=None):
        check_detect_args(_shape_of(data), self.npixels, self.connectivity, _shape_of(threshold),
                          None if mask is None else _shape_of(mask))
        _B.require_gpu()
        d, batched = _to_dev(data)
        lab, n = _detect_dev(d, threshold, self.npixels, self.connectivity, mask)
        if not batched and n[0] == 0:
            warnings.warn("No sources were found.", NoDetectionsWarning)
            return None
        if self.deblend:
            return _deblended_image(_deblend_dev(d.to(_B.torch.float64), lab, n, self.npixels,
                                                 self.nlevels, self.contrast, self.mode,
                                                 self.connectivity,
                                                 large_parents=self.large_parents),
                                    batched, self.device_out)
        return SegmentationImage(_out(lab, batched, self.device_out), n, batched)


def shape_columns(sigx2, sigxy, sigy2):
    """The shape columns from the covariance of a segment's convolved pixels,
    by the formulas of photutils' documentation: a^2 and b^2 are the
    eigenvalues of [[sigx2, sigxy], [sigxy, sigy2]] (negative rounding residue
    clipped to 0), orientation = atan2(2 sigxy, sigx2 - sigy2) / 2 in degrees
    (counterclockwise from +x), eccentricity = sqrt(1 - b^2 / a^2),
    ellipticity = 1 - b / a, fwhm = 2 sqrt(ln 2 (a^2 + b^2))."""
    sx, sxy, sy = (np.asarray(v, dtype=np.float64) for v in (sigx2, sigxy, sigy2))
    half, root = (sx + sy) / 2, np.sqrt(((sx - sy) / 2) ** 2 + sxy ** 2)
    a2, b2 = np.maximum(half + root, 0.0), np.maximum(half - root, 0.0)
    a, b = np.sqrt(a2), np.sqrt(b2)
    with np.errstate(invalid="ignore", divide="ignore"):
        ecc, ell = np.sqrt(1.0 - b2 / a2), 1.0 - b / a
    return dict(semimajor_sigma=a, semiminor_sigma=b,
                orientation=np.degrees(0.5 * np.arctan2(2.0 * sxy, sx - sy)),
                eccentricity=ecc, ellipticity=ell, fwhm=2.0 * np.sqrt(np.log(2.0) * (a2 + b2)))


class SourceCatalog:
    """``SourceCatalog(data, segment_img, convolved_data=None, localbkg_width=0)``
    on the device.

    ``data`` is already background-subtracted, as ``source_info`` passes it
    (``background`` is accepted for photutils' signature and only kept).
    ``segment_img``: a :class:`SegmentationImage` or an integer label image.
    Attributes, one entry per label (a batch: a list of B arrays each):
    ``label``, ``area``, ``bbox_xmin`` / ``bbox_xmax`` / ``bbox_ymin`` /
    ``bbox_ymax`` (inclusive), ``segment_flux``, ``min_value``, ``max_value`` (of
    ``data``), ``xcentroid``, ``ycentroid``, ``covar_sigx2`` / ``covar_sigxy`` /
    ``covar_sigy2`` (first and central second moments of ``convolved_data``, or
    of ``data`` without one) and from those ``semimajor_sigma``,
    ``semiminor_sigma``, ``orientation`` (degrees), ``eccentricity``,
    ``ellipticity``, ``fwhm`` (:func:`shape_columns`).  ``segment_flux_sum`` is
    the numpy sum of ``segment_flux`` over all segments per image -- what the
    application uses; at ``localbkg_width=0`` deblending does not change it.  The columns describe the segments of
    ``segment_img``, deblended or not; the moment and shape columns are modelled on photutils, not pinned to it.
    ``localbkg_width > 0`` (photutils' parameter; the reference passes 5) adds
    the column ``local_background`` -- SExtractor's mode of the sigma-clipped
    unlabelled pixels of a rectangular annulus of that width around the
    source's box -- and subtracts it from
    ``segment_flux`` (times ``area``), ``min_value`` and ``max_value``; the
    other columns are unaffected.  A source with fewer than 10 annulus values
    gets 0.0; one with more than ``LOCALBKG_MAX`` gets 0.0, no correction and a
    :class:`LocalBackgroundCapWarning`; ``localbkg_status`` holds the
    ``BSGP_LOCALBKG_*`` bits per image and ``localbkg_npix`` [n, 2] the annulus
    values gathered and those the clipping left, per source.  At the default 0 ``local_background``
    raises ``KeyError``; ``sky_centroid`` and ``segment_fluxerr`` always do,
    with the reason.  ``device_out=True`` adds ``int_cols`` / ``f64_cols`` (CUDA
    tensors [B, cap, 5] / [B, cap, 8]) and, with a width,
    ``local_background_dev`` [B, cap].  A catalogue made by
    ``source_info(..., validate=True)`` also has the bool column ``valid``,
    ``validation`` and ``segment_flux_sum_valid``."""

    def __init__(self, data, segment_img, convolved_data=None, background=None, device_out=False,
                 localbkg_width=0):
        torch = _B.torch
        shape = _shape_of(data)
        _check_image_shape(shape)
        width = check_localbkg_width(localbkg_width)
        seg = segment_img.data if isinstance(segment_img, SegmentationImage) else segment_img
        if _shape_of(seg) != shape:
            raise ValueError(f"segment_img shape {_shape_of(seg)} does not match data shape {shape}")
        if convolved_data is not None and _shape_of(convolved_data) != shape:
            raise ValueError(f"convolved_data shape {_shape_of(convolved_data)} does not match "
                             f"data shape {shape}")
        _B.require_gpu()
        d, batched = _to_dev(data, keep_f32=False)
        c = None if convolved_data is None else _to_dev(convolved_data, keep_f32=False)[0]
        lab = seg if torch.is_tensor(seg) else torch.from_numpy(np.ascontiguousarray(seg))
        lab = lab.to(device="cuda", dtype=torch.int32).contiguous()
        lab = lab if batched else lab[None]
        if isinstance(segment_img, SegmentationImage):
            n = np.asarray(segment_img._n, dtype=np.int32)
        else:
            if bool((lab < 0).any()):
                raise ValueError("segment_img holds negative labels")
            n = lab.reshape(lab.shape[0], -1).amax(dim=1).cpu().numpy().astype(np.int32)
        self._fill(d, c, lab, n, batched, device_out, width)
        self.background = background

    def _fill(self, d, c, lab, n, batched, device_out, localbkg_width=0.0, validate=None):
        """validate: None, or (image, bkgmap, rmsmap, (ny, nx)) on the device --
        the unsubtracted image and its maps: the rows are validated from their
        centroid columns in place."""
        torch = _B.torch
        B, H, W = d.shape
        cap = max(1, int(n.max()))
        nd = torch.from_numpy(np.ascontiguousarray(n)).to("cuda")
        ic = torch.empty((B, cap, 5), dtype=torch.int32, device="cuda")
        fc = torch.empty((B, cap, 8), dtype=torch.float64, device="cuda")
        st = torch.empty((B,), dtype=torch.int32, device="cuda")
        _B.check(_B.lib().bsgp_segment_catalog(_B._ptr(d), _B._ptr(c), _B._ptr(lab), B, H, W, cap,
                                               _B._ptr(nd), _B._ptr(ic), _B._ptr(fc), _B._ptr(st),
                                               _B.current_stream()))
        lbd = None
        if localbkg_width > 0:  # L1 to L6: corrects fc in place (stream-ordered after the catalogue)
            lbd = torch.empty((B, cap), dtype=torch.float64, device="cuda")
            npx = torch.empty((B, cap, 2), dtype=torch.int32, device="cuda")
            lst = torch.empty((B,), dtype=torch.int32, device="cuda")
            _B.check(_B.lib().bsgp_segment_local_background(
                _B._ptr(d), _dtype(d), _B._ptr(lab), B, H, W, cap, _B._ptr(nd), _B._ptr(ic),
                _B._ptr(fc), float(localbkg_width), LOCALBKG_SIGMA, LOCALBKG_MAXITERS,
                LOCALBKG_MIN_PIXELS, 1, _B._ptr(lbd), _B._ptr(npx), _B._ptr(lst),
                _B.current_stream()))
        val = None
        if validate is not None:  # V1 to V6 from the centroid columns (stream-ordered, no copy)
            img, bg, rms, (vh, vw) = validate
            val = _validate_dev(img, bg, rms, ctypes.c_void_p(fc.data_ptr() + 3 * 8), 8, nd, cap,
                                vh, vw, 3.0)
        ich, fch, sth = ic.cpu().numpy(), fc.cpu().numpy(), st.cpu().numpy()
        if sth.any():
            raise _B.BsgpError(_B.BSGP_ERR_ARG, f"image {int(np.flatnonzero(sth)[0])}: labels "
                               "outside 1..nlabels in the segmentation image")
        self.batched, self.nlabels = batched, (n if batched else int(n[0]))
        if device_out:
            self.int_cols, self.f64_cols = ic, fc
        cols = {"label": [np.arange(1, k + 1, dtype=np.int32) for k in n]}
        for j, nm in enumerate(INT_COLUMNS):
            cols[nm] = [ich[b, :n[b], j] for b in range(B)]
        for j, nm in enumerate(F64_COLUMNS):
            cols[nm] = [fch[b, :n[b], j] for b in range(B)]
        shp = [shape_columns(fch[b, :n[b], 5], fch[b, :n[b], 6], fch[b, :n[b], 7]) for b in range(B)]
        for nm in SHAPE_COLUMNS:
            cols[nm] = [s[nm] for s in shp]
        self.localbkg_width = localbkg_width
        if lbd is not None:
            lbh, nph, lsh = lbd.cpu().numpy(), npx.cpu().numpy(), lst.cpu().numpy()
            cols["local_background"] = [lbh[b, :n[b]] for b in range(B)]
            npl = [nph[b, :n[b]] for b in range(B)]
            self.localbkg_npix = npl if batched else npl[0]
            self.localbkg_status = lsh if batched else int(lsh[0])
            if device_out:
                self.local_background_dev = lbd
            if (lsh & _B.BSGP_LOCALBKG_OVER_CAP).any():
                over = sum(int((v[:, 0] > LOCALBKG_MAX).sum()) for v in npl)
                warnings.warn(f"{over} source(s) with a local-background annulus of more than "
                              f"{LOCALBKG_MAX} values were left uncorrected (local_background 0)",
                              LocalBackgroundCapWarning)
        self._cols = cols
        # one fixed order for the total as well: numpy's sum of the per-segment fluxes
        tot = np.array([float(np.sum(v)) for v in cols["segment_flux"]])
        self.segment_flux_sum = tot if batched else float(tot[0])
        if val is not None:
            stats, valid, status = val
            self.validation = SourceValidation(valid.cpu().numpy(), stats.cpu().numpy(),
                                               status.cpu().numpy(), n, batched)
            if device_out:
                self.validation.valid_dev, self.validation.stats_dev = valid, stats
                self.validation.status_dev = status
            ok = self.validation.valid if batched else [self.validation.valid]
            cols["valid"] = list(ok)
            tot = np.array([float(np.sum(f[v])) for f, v in zip(cols["segment_flux"], ok)])
            self.segment_flux_sum_valid = tot if batched else float(tot[0])

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        try:
            return self[name]
        except KeyError as e:
            raise AttributeError(str(e)) from None

    def __getitem__(self, name):
        if name not in self._cols and name in UNAVAILABLE:
            raise KeyError(f"{name} is not available: {UNAVAILABLE[name]}")
        if name not in self._cols:
            raise KeyError(f"unknown column {name!r}; available: {', '.join(COLUMNS)}")
        v = self._cols[name]
        return v if self.batched else v[0]

    def __len__(self):
        return int(np.sum(self.nlabels))

    def to_dict(self, columns=None):
        """The named columns (default: all) as a dict; unknown and unavailable
        names raise ``KeyError``."""
        every = COLUMNS + tuple(k for k in ("local_background", "valid") if k in self._cols)
        return {k: self[k] for k in (every if columns is None else columns)}


def source_info(data, box_size, n_pixels=5, sigma_threshold=1.5, device_out=False, deblend=False,
                nlevels=32, contrast=0.001, large_parents=False, validate=False, validate_size=100,
                localbkg_width=0):
    """``utils.source_info`` (restoration/utils.py:235-247) for an image or a
    batch, with its deblending on request: ``Background2D(data, box_size,
    filter_size=(3, 3))``, ``sub = data - background``, ``threshold =
    sigma_threshold * background_rms``, ``conv = convolve(sub,
    make_2dgaussian_kernel(1.2, 3))``, ``detect_sources(conv, threshold,
    n_pixels)``, with ``deblend=True`` the reference's
    ``SourceFinder(npixels=n_pixels, deblend=True)``, i.e. ``deblend_sources(conv,
    segment_img, n_pixels, nlevels=nlevels, contrast=contrast)`` (connectivity 8,
    mode 'exponential'), and the catalogue of ``sub`` with
    ``convolved_data=conv``.  At ``localbkg_width=0`` the default
    ``deblend=False`` gives the same sum of ``segment_flux`` and the columns of
    undeblended segments.  ``localbkg_width`` as in :class:`SourceCatalog`; the
    reference's catalogue (utils.py:244-246) is ``localbkg_width=5`` with
    ``deblend=True``, and with a width the sum depends on the deblending.
    ``large_parents=True`` also deblends the segments whose box is over
    ``DEBLEND_MAX_BOX`` (crowded cores), as in :func:`deblend_sources`.
    Returns ``(catalog, bkg)``; the catalogue also carries ``segment_img``,
    ``data`` (sub) and ``convolved_data``.  An unbatched image without a
    detection warns and gives ``(None, bkg)``.  With ``device_out=True`` the
    maps stay on the device.

    ``validate=True`` runs the reference's ``validation_source``
    (utils.py:313-329; :func:`validate_sources`) on every row,
    at its centroid, with the unsubtracted ``data``, ``bkg.background`` and
    ``bkg.background_rms`` as they are on the device and windows of
    ``validate_size``: the catalogue gains the bool column ``valid``, the
    attribute ``validation`` (a :class:`SourceValidation`) and
    ``segment_flux_sum_valid``, numpy's sum of ``segment_flux`` over the valid
    rows.  No row is dropped: the labels stay those of ``segment_img``.  A row
    with a NaN centroid is invalid (``BSGP_STAMP_BAD_POSITION``).  The default
    ``False`` leaves every output as it is without the parameter."""
    from background import Background2D
    torch = _B.torch
    _check_image_shape(_shape_of(data))
    vsize = None
    if validate:
        shp = _shape_of(data)
        vsize = check_validate_args(shp, shp, shp, validate_size)
    check_detect_args(_shape_of(data), n_pixels, 8)
    check_deblend_args(_shape_of(data), _shape_of(data), n_pixels, nlevels, contrast,
                       large_parents=large_parents)
    width = check_localbkg_width(localbkg_width)
    bkg = Background2D(data, box_size, filter_size=(3, 3), device_out=True)
    d, batched = _to_dev(data)
    bg = bkg.background if batched else bkg.background[None]
    rms = bkg.background_rms if batched else bkg.background_rms[None]
    sub = d.to(torch.float64) - bg
    thr = float(sigma_threshold) * rms
    if not bool(torch.isfinite(sub).all()):
        raise ValueError("data holds non-finite pixels: NaN interpolation is not offered")
    conv = _convolve_dev(sub, make_2dgaussian_kernel(1.2, 3))
    lab, n = _detect_dev(conv, thr, int(n_pixels), 8, None)
    if not device_out:
        for nm in ("background", "background_rms", "background_mesh", "background_rms_mesh"):
            setattr(bkg, nm, getattr(bkg, nm).cpu().numpy())
    if not batched and n[0] == 0:
        warnings.warn("No sources were found.", NoDetectionsWarning)
        return None, bkg
    seg = None
    if deblend:
        res = _deblend_dev(conv, lab, n, int(n_pixels), nlevels, contrast, "exponential", 8,
                           large_parents=bool(large_parents))
        seg, (lab, n) = _deblended_image(res, batched, device_out), res[:2]
    cat = SourceCatalog.__new__(SourceCatalog)
    cat._fill(sub, conv, lab, n.astype(np.int32), batched, device_out, width,
              validate=(d, bg, rms, vsize) if validate else None)
    cat.background = None
    cat.segment_img = seg or SegmentationImage(_out(lab, batched, device_out), n, batched)
    cat.data, cat.convolved_data = _out(sub, batched, device_out), _out(conv, batched, device_out)
    return cat, bkg


def segment_flux_sums(images, box_size, n_pixels=5, sigma_threshold=1.5, localbkg_width=0,
                      deblend=False, large_parents=False):
    """Sum of ``segment_flux`` per image of a batch [B, H, W] (one batched
    ``source_info``); 0.0 for an image without a detection.  ``localbkg_width``,
    ``deblend`` and ``large_parents`` as in :func:`source_info`
    (``localbkg_width=5, deblend=True``: the reference's sum)."""
    cat, _ = source_info(images, box_size, n_pixels, sigma_threshold, device_out=True,
                         deblend=deblend, large_parents=large_parents,
                         localbkg_width=localbkg_width)
    return np.asarray(cat.segment_flux_sum, dtype=np.float64)


def flux_fraction_score(gn, box_size=60, n_pixels_orig=5, n_pixels_restored=1,
                        sigma_threshold=1.5):
    """The application's beta-candidate score
    (application_sgp_subdivisions.py:92-99) as a callable for the ``score=``
    parameters of ``sgp_betaDiv_multistart`` and
    ``sgp_subdivisions_multistart``: ``score(x)`` and ``score(x, tile)`` return
    ``1 - sum(segment_flux(source_info(x, box_size, n_pixels_restored))) /
    sum(segment_flux(source_info(gn or tile, box_size, n_pixels_orig)))``;
    ``score.batch(xs)`` / ``score.batch(xs, tiles)`` evaluate candidates
    [n, H, W] in one batched ``source_info`` (``tiles``: one observed image, or
    one per candidate).  The catalogues are those of ``localbkg_width=0``
    without deblending; :func:`catalog_flux_fraction_score` takes both."""
    return catalog_flux_fraction_score(gn, box_size, n_pixels_orig, n_pixels_restored,
                                       sigma_threshold)


def catalog_flux_fraction_score(gn, box_size=60, n_pixels_orig=5, n_pixels_restored=1,
                                sigma_threshold=1.5, localbkg_width=0, deblend=False):
    """:func:`flux_fraction_score` with the catalogue's keywords:
    ``localbkg_width`` and ``deblend`` go to both ``source_info`` calls.  The
    reference's score is ``localbkg_width=5, deblend=True`` (its catalogue
    subtracts a local background, utils.py:244-246); the defaults give
    :func:`flux_fraction_score`."""
    check_localbkg_width(localbkg_width)
    cache = {}
    kw = dict(localbkg_width=localbkg_width, deblend=deblend)

    def orig(img):
        """Flux sums of the observed image(s) [n, H, W] or [H, W] -> [n] or [1]."""
        a = img if len(_shape_of(img)) == 3 else img[None]
        return segment_flux_sums(a, box_size, n_pixels_orig, sigma_threshold, **kw)

    def orig_gn():
        if "gn" not in cache:
            if gn is None:
                raise ValueError("flux_fraction_score(None) needs the observed tile: score(x, tile)")
            cache["gn"] = orig(gn)
        return cache["gn"]

    def batch(xs, tiles=None):
        den = orig_gn() if tiles is None else orig(tiles)
        num = segment_flux_sums(xs, box_size, n_pixels_restored, sigma_threshold, **kw)
        return 1.0 - num / den

    def score(x, tile=None):
        return float(batch(x[None], tile)[0])

    score.batch = batch
    return score


# ---- validation of detected sources (bsgp_validate_sources) ----
VALIDATE_MAX = _B.BSGP_VALIDATE_MAX


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def check_validate_args(image_shape, bkgmap_shape, rmsmap_shape, size=100, nsigma=3.0,
                        positions_shape=None):
    """The argument checks of validate_sources (host only; nothing touches the
    GPU): the image is [H, W] or [B, H, W]; both maps have one shape, [H, W]
    or (for a batch) [B, H, W]; ``size`` is a positive int or a pair (ny, nx)
    of them with ``ny * nx <= VALIDATE_MAX``; ``nsigma`` is a number, not NaN;
    ``positions_shape`` (when given) is the shape [n, 2] of the positions of an
    image, or for a batch a list of B such shapes.  Returns (ny, nx)."""
    shape = tuple(image_shape)
    _check_image_shape(shape, "image")
    for nm, s in (("bkgmap", tuple(bkgmap_shape)), ("rmsmap", tuple(rmsmap_shape))):
        if s != shape[-2:] and not (len(shape) == 3 and s == shape):
            raise ValueError(f"{nm} shape {s} does not match image shape {shape}: the maps are "
                             "[H, W] or, for a batch, [B, H, W]")
    if tuple(bkgmap_shape) != tuple(rmsmap_shape):
        raise ValueError(f"bkgmap shape {tuple(bkgmap_shape)} and rmsmap shape "
                         f"{tuple(rmsmap_shape)} differ")
    sz = (size, size) if np.ndim(size) == 0 else tuple(np.asarray(size).tolist())
    if len(sz) != 2 or not all(_is_number(v) and int(v) == v and v >= 1 for v in sz):
        raise ValueError(f"size must be an int >= 1 or a pair (ny, nx) of them, got {size!r}")
    sh, sw = int(sz[0]), int(sz[1])
    if sh * sw > VALIDATE_MAX:
        raise ValueError(f"size {size!r}: a window of {sh * sw} values, the device holds at most "
                         f"VALIDATE_MAX = {VALIDATE_MAX} (128 x 128)")
    if not _is_number(nsigma) or np.isnan(nsigma):
        raise ValueError(f"nsigma must be a number, got {nsigma!r}")
    if positions_shape is not None:
        if len(shape) == 3:
            if not isinstance(positions_shape, list) or len(positions_shape) != shape[0]:
                raise ValueError(f"a batch of {shape[0]} images needs a list of {shape[0]} position "
                                 "arrays")
            shapes = positions_shape
        else:
            if isinstance(positions_shape, list):
                raise ValueError("a list of positions needs a batch of images [B, H, W]")
            shapes = [positions_shape]
        for s in shapes:
            if len(tuple(s)) != 2 or tuple(s)[1] != 2:
                raise ValueError(f"positions must be [n, 2] in (x, y), got shape {tuple(s)}")
    return sh, sw


class SourceValidation:
    """Result of :func:`validate_sources`, one entry per source: ``valid``
    (bool: ``source_pixs > bkg + nsigma * rms``), ``source_pixs`` (the mean of
    the window's three largest image values), ``bkg`` (the median of the
    background window), ``rms`` (the mean of the rms window) and ``status``
    (``BSGP_STAMP_PARTIAL`` where the window leaves the frame;
    ``BSGP_STAMP_NO_OVERLAP`` / ``BSGP_STAMP_BAD_POSITION``: invalid, NaN
    statistics).  For a batch every attribute is a list over the images.  With
    ``device_out=True`` the entries are CUDA tensors (views of ``valid_dev``
    [B, cap] int32, ``stats_dev`` [B, cap, 3] and ``status_dev`` [B, cap])."""

    def __init__(self, valid, stats, status, n, batched):
        cols = dict(valid=[], source_pixs=[], bkg=[], rms=[], status=[])
        for b, k in enumerate(n):
            cols["valid"].append(valid[b, :k] != 0)
            cols["source_pixs"].append(stats[b, :k, 0])
            cols["bkg"].append(stats[b, :k, 1])
            cols["rms"].append(stats[b, :k, 2])
            cols["status"].append(status[b, :k])
        self.batched = batched
        for k, v in cols.items():
            setattr(self, k, v if batched else v[0])


def _validate_dev(d, bg, rms, xy, xy_stride, nd, cap, sh, sw, nsigma):
    """(stats [B, cap, 3], valid [B, cap], status [B, cap]) CUDA tensors of
    bsgp_validate_sources; asynchronous.  d: CUDA [B, H, W]; bg, rms: float64
    CUDA [H, W] or [B, H, W]; xy: the pointer of the first (x, y); nd: int32
    CUDA [B]."""
    torch = _B.torch
    B, H, W = d.shape
    stats = torch.empty((B, cap, 3), dtype=torch.float64, device="cuda")
    valid = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    status = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    _B.check(_B.lib().bsgp_validate_sources(
        _B._ptr(d), _dtype(d), _B._ptr(bg), _B._ptr(rms), B, H, W, int(bg.dim() == 3), xy,
        int(xy_stride), _B._ptr(nd), int(cap), int(sh), int(sw), float(nsigma), _B._ptr(stats),
        _B._ptr(valid), _B._ptr(status), _B.current_stream()))
    return stats, valid, status


def _positions_of(p):
    """[n, 2] float64 host array of one image's positions: an array in (x, y),
    or anything with ``xcentroid`` / ``ycentroid`` columns."""
    if isinstance(p, SourceCatalog) or isinstance(p, dict) or hasattr(p, "keys"):
        if getattr(p, "batched", False):
            raise ValueError("a batch is a list of unbatched catalogues")
        x, y = _column(p, "xcentroid"), _column(p, "ycentroid")
        if x is None or y is None:
            raise ValueError("a catalogue needs the columns 'xcentroid' and 'ycentroid'")
        return np.stack([x.astype(np.float64).reshape(-1), y.astype(np.float64).reshape(-1)], axis=1)
    a = np.asarray(p, dtype=np.float64)
    return a.reshape(0, 2) if a.size == 0 and a.ndim < 2 else a


def validate_sources(image, positions, bkgmap, rmsmap, size=100, nsigma=3.0, device_out=False):
    """The reference's ``utils.validation_source`` (restoration/utils.py:313-329)
    for every source of an image or of a batch, on the device
    (``bsgp_validate_sources``): a source is valid when
    the mean of the three largest pixels of the ``size`` window around it
    exceeds the window's median background by ``nsigma`` times its mean rms.

    ``image`` ([H, W] or [B, H, W], float32 or float64) must not be
    background-subtracted.  ``positions``: an array [n, 2] in (x, y), a
    :class:`SourceCatalog` (its ``xcentroid`` / ``ycentroid``; one made with
    ``device_out=True`` is read from its device columns, nothing is copied),
    or for a batch a list of B arrays or unbatched catalogues, or a batched
    :class:`SourceCatalog`.  ``bkgmap`` / ``rmsmap``: [H, W] for all images or
    [B, H, W]; they are widened to float64.  ``size``: an int or (ny, nx), at
    most ``VALIDATE_MAX`` cells.  The window is ``Cutout2D``'s in mode
    'partial' with ``fill_value=0.0``: cells outside the frame are 0.0 and take
    part in the statistics, as in the reference.  A position whose window
    misses the frame, or that is not finite, is invalid with NaN statistics and
    a status bit (astropy raises).  Returns a :class:`SourceValidation`."""
    torch = _B.torch
    shape = _shape_of(image)
    _check_image_shape(shape, "image")
    in_place = isinstance(positions, SourceCatalog) and hasattr(positions, "f64_cols")
    if in_place:
        if positions.batched != (len(shape) == 3) or \
                (positions.batched and len(positions.nlabels) != shape[0]):
            raise ValueError("the catalogue and the image differ in their batch")
        sh, sw = check_validate_args(shape, _shape_of(bkgmap), _shape_of(rmsmap), size, nsigma)
        n = np.atleast_1d(np.asarray(positions.nlabels, dtype=np.int32))
    else:
        if isinstance(positions, SourceCatalog) and positions.batched:
            positions = [{"xcentroid": x, "ycentroid": y}
                         for x, y in zip(positions["xcentroid"], positions["ycentroid"])]
        # a list is a batch only beside a batch of images: [[x, y], ...] is one image's array
        pos = [_positions_of(p) for p in positions] \
            if isinstance(positions, list) and len(shape) == 3 else _positions_of(positions)
        sh, sw = check_validate_args(shape, _shape_of(bkgmap), _shape_of(rmsmap), size, nsigma,
                                     [p.shape for p in pos] if isinstance(pos, list) else pos.shape)
        pos = pos if isinstance(pos, list) else [pos]
        n = np.array([len(p) for p in pos], dtype=np.int32)
    _B.require_gpu()
    d, batched = _to_dev(image)
    bg, rm = (_to_dev(m, keep_f32=False)[0] for m in (bkgmap, rmsmap))
    if len(_shape_of(bkgmap)) == 2:
        bg, rm = bg[0], rm[0]
    if in_place:
        fc = positions.f64_cols
        cap, xy, stride = int(fc.shape[1]), ctypes.c_void_p(fc.data_ptr() + 3 * 8), 8
        keep = fc
    else:
        cap = max(1, int(n.max()))
        host = np.zeros((len(pos), cap, 2))
        for b, p in enumerate(pos):
            host[b, :len(p)] = p
        keep = torch.from_numpy(host).to("cuda")
        xy, stride = _B._ptr(keep), 2
    nd = torch.from_numpy(np.ascontiguousarray(n)).to("cuda")
    stats, valid, status = _validate_dev(d, bg, rm, xy, stride, nd, cap, sh, sw, nsigma)
    if device_out:
        out = SourceValidation(valid, stats, status, n, batched)
        out.valid_dev, out.stats_dev, out.status_dev = valid, stats, status
        out._keep = (d, bg, rm, keep, nd)
        return out
    vh, sth, sh_ = valid.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy()  # waits
    return SourceValidation(vh, sth, sh_, n, batched)


def validation_source(image, coord, bkgmap, rmsmap, size=100):
    """``utils.validation_source(image, coord, bkgmap, rmsmap, size=100)``
    (restoration/utils.py:313-329) for one source at ``coord = (x, y)``: a
    Python ``bool``, the ``valid`` of the one-row :func:`validate_sources`."""
    pos = np.asarray(coord, dtype=np.float64).reshape(1, 2)
    return bool(validate_sources(image, pos, bkgmap, rmsmap, size=size).valid[0])


# ---- cross-match of two catalogues (bsgp_match_catalogs) ----
MATCH_LDS_MAX, MATCH_MAX = _B.BSGP_MATCH_LDS_MAX, _B.BSGP_MATCH_MAX
MATCH_PATHS = {None: _B.BSGP_MATCH_AUTO, "auto": _B.BSGP_MATCH_AUTO, "lds": _B.BSGP_MATCH_LDS,
               "global": _B.BSGP_MATCH_GLOBAL}
METRIC_COLUMNS = ("segment_flux", "fwhm", "ellipticity")


def check_match_args(max_sep, path=None, batch1=1, batch2=1, cap1=1, cap2=1):
    """The argument checks of match_catalogs (host only): ``max_sep`` a finite
    number >= 0, ``path`` None / 'auto', 'lds' or 'global', both sides of one
    batch size, at most ``MATCH_MAX`` rows per catalogue and, on the LDS path,
    ``MATCH_LDS_MAX`` rows in both.  Returns (max_sep, the path's code)."""
    s = max_sep
    if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, float, np.integer, np.floating)) \
            or not np.isfinite(s) or s < 0:
        raise ValueError(f"max_sep must be a finite number >= 0, got {max_sep!r}")
    if not isinstance(path, (str, type(None))) or path not in MATCH_PATHS:
        raise ValueError(f"path must be None, 'auto', 'lds' or 'global', got {path!r}")
    if batch1 != batch2:
        raise ValueError(f"the catalogues are batches of {batch1} and {batch2} images: both sides "
                         "must have the same batch size")
    if max(cap1, cap2) > MATCH_MAX:
        raise ValueError(f"catalogues of {cap1} and {cap2} rows: a catalogue holds at most "
                         f"{MATCH_MAX}")
    if path == "lds" and cap1 + cap2 > MATCH_LDS_MAX:
        raise ValueError(f"catalogues of {cap1} + {cap2} rows: path='lds' holds at most "
                         f"{MATCH_LDS_MAX} in both")
    return float(s), MATCH_PATHS[path]


def _match_items(cat):
    """(the images of a catalogue as a list of unbatched catalogues, whether it
    is a batch).  A list is a batch, a SourceCatalog what it was made as."""
    if isinstance(cat, SourceCatalog) and cat.batched:
        return [{k: cat[k][b] for k in ("xcentroid", "ycentroid", "area", "label")}
                for b in range(len(cat.nlabels))], True
    if isinstance(cat, list):
        if any(isinstance(c, list) or getattr(c, "batched", False) for c in cat):
            raise ValueError("a batch is a list of unbatched catalogues")
        return cat, True
    return [cat], False


def _column(cat, name):
    try:
        v = cat[name]
    except (KeyError, TypeError, IndexError, ValueError):
        return None
    return np.asarray(getattr(v, "value", v))


def _xy_of(cat):
    """(x, y, area or None, label or None) of one unbatched catalogue: an
    (x, y) tuple, or anything indexable by 'xcentroid' / 'ycentroid' (and,
    where it has them, 'area' and 'label')."""
    if isinstance(cat, tuple):
        if len(cat) != 2:
            raise ValueError(f"a coordinate tuple is (x, y), got {len(cat)} entries")
        x, y, area, label = np.asarray(cat[0]), np.asarray(cat[1]), None, None
    else:
        x, y = _column(cat, "xcentroid"), _column(cat, "ycentroid")
        if x is None or y is None:
            raise ValueError("a catalogue is a SourceCatalog, an (x, y) tuple or indexable by "
                             f"'xcentroid' / 'ycentroid', got {type(cat).__name__}")
        area, label = _column(cat, "area"), _column(cat, "label")
    x, y = x.astype(np.float64).reshape(-1), y.astype(np.float64).reshape(-1)
    if x.shape != y.shape or (area is not None and area.shape != x.shape):
        raise ValueError(f"the columns of a catalogue differ in length ({len(x)} x, {len(y)} y)")
    return x, y, area, label


class _MatchSide:
    """One side of a match on the device: column pointers as
    bsgp_match_catalogs takes them, the host row counts and the labels."""

    def __init__(self, cat):
        torch = _B.torch
        if isinstance(cat, SourceCatalog) and hasattr(cat, "f64_cols"):
            # device columns (bsgp_segment_catalog's layout), matched in place
            fc, ic = cat.f64_cols, cat.int_cols
            self.batched = cat.batched
            self.n = np.atleast_1d(np.asarray(cat.nlabels, dtype=np.int32))
            self.B, self.cap = int(fc.shape[0]), int(fc.shape[1])
            self.x = ctypes.c_void_p(fc.data_ptr() + 3 * 8)
            self.y = ctypes.c_void_p(fc.data_ptr() + 4 * 8)
            self.valid, self.stride, self.vstride = _B._ptr(ic), 8, 5
            self.labels = [np.arange(1, k + 1, dtype=np.int32) for k in self.n]
            self._keep = (fc, ic)
        else:
            items, self.batched = _match_items(cat)
            cols = [_xy_of(c) for c in items]
            self.B = len(cols)
            self.n = np.array([len(c[0]) for c in cols], dtype=np.int32)
            self.cap = max(1, int(self.n.max())) if self.B else 1
            xy = np.zeros((2, self.B, self.cap))
            va = None if all(c[2] is None for c in cols) else np.ones((self.B, self.cap), np.int32)
            for b, c in enumerate(cols):
                xy[0, b, :len(c[0])], xy[1, b, :len(c[0])] = c[0], c[1]
                if c[2] is not None:
                    va[b, :len(c[0])] = np.asarray(c[2]) > 0
            xyd = torch.from_numpy(xy).to("cuda")
            vad = None if va is None else torch.from_numpy(va).to("cuda")
            self.x, self.y = _B._ptr(xyd[0]), _B._ptr(xyd[1])
            self.valid, self.stride, self.vstride = _B._ptr(vad), 1, 1
            self.labels = [c[3] for c in cols]
            self._keep = (xyd, vad)
        self.nd = torch.from_numpy(np.ascontiguousarray(self.n)).to("cuda")

    def args(self):
        return (self.x, self.y, self.stride, self.valid, self.vstride, self.cap, _B._ptr(self.nd))


class CatalogMatch:
    """Result of :func:`match_catalogs`.  ``idx1`` / ``idx2``: the 0-based rows
    of the pairs in catalogue 1 / 2, ordered by ``idx1`` (the order of the
    reference's published tables); ``separation`` of each pair; ``n_pairs``;
    ``unmatched1`` / ``unmatched2``: the rows without a partner (rows that took
    no part included); ``match1`` / ``match2``: per row the partner's row or
    -1; ``sep1``: per row of catalogue 1 the separation or NaN; ``labels1`` /
    ``labels2``: the pairs' labels where the catalogue has ``label`` (else
    ``None``); ``status``: the ``BSGP_MATCH_*`` bits.  For a batch every
    attribute is a list over the images (``n_pairs`` and ``status`` int
    arrays).  With ``device_out=True`` ``match1_dev`` / ``match2_dev`` /
    ``sep1_dev`` [B, cap] and ``n_pairs_dev`` / ``status_dev`` [B] are the CUDA
    tensors the kernel wrote."""

    def __init__(self, match1, match2, sep1, status, labels1=None, labels2=None, batched=False):
        B = len(match1)
        labels1, labels2 = labels1 or [None] * B, labels2 or [None] * B
        cols = {k: [] for k in ("idx1", "idx2", "separation", "unmatched1", "unmatched2",
                                "labels1", "labels2")}
        for m1, m2, sp, l1, l2 in zip(match1, match2, sep1, labels1, labels2):
            i = np.flatnonzero(m1 >= 0)
            cols["idx1"].append(i), cols["idx2"].append(m1[i].astype(np.int64))
            cols["separation"].append(sp[i])
            cols["unmatched1"].append(np.flatnonzero(m1 < 0))
            cols["unmatched2"].append(np.flatnonzero(m2 < 0))
            cols["labels1"].append(None if l1 is None else np.asarray(l1)[i])
            cols["labels2"].append(None if l2 is None else np.asarray(l2)[m1[i]])
        cols.update(match1=list(match1), match2=list(match2), sep1=list(sep1))
        self.batched = batched
        for k, v in cols.items():
            setattr(self, k, v if batched else v[0])
        n = np.array([len(i) for i in cols["idx1"]], dtype=np.int64)
        st = np.asarray(status, dtype=np.int32)
        self.n_pairs, self.status = (n, st) if batched else (int(n[0]), int(st[0]))


def match_catalogs(cat1, cat2, max_sep=1.1, device_out=False, path=None):
    """Cross-match two source catalogues by position on the device: the greedy
    symmetric best match within ``max_sep`` pixels (``bsgp_match_catalogs``;
    DESIGN §3.10, M1 to M6).  The candidates -- pairs with ``sqrt(dx^2 + dy^2)
    <= max_sep`` -- are taken in the order of (squared distance, row of
    catalogue 1, row of catalogue 2), a pair being accepted iff neither row is
    taken.  With catalogue 1 the restored and catalogue 2 the original
    catalogue and the default 1.1 this is the reference's published
    ``results/*_MATCHED.csv``.

    A catalogue is a :class:`SourceCatalog` (batched or not; one made with
    ``device_out=True`` is matched from its device columns, no column is
    copied), anything indexable by ``'xcentroid'`` / ``'ycentroid'`` (a dict, a
    DataFrame, a table), an ``(x, y)`` tuple, or a list of those for a batch;
    both sides must have one batch size.  A tuple is always one (x, y) pair, a
    list always a batch.  Rows whose ``area`` is not > 0 (a SourceCatalog's
    absent labels; any catalogue with that column) and rows with a non-finite
    coordinate take no part.
    ``path``: None / 'auto', 'lds' (both catalogues in LDS, at most
    ``MATCH_LDS_MAX`` rows together) or 'global' (at most ``MATCH_MAX`` rows
    each); the result does not depend on it.  Returns a :class:`CatalogMatch`."""
    torch = _B.torch
    (i1, b1), (i2, b2) = _match_items(cat1), _match_items(cat2)
    if b1 != b2:
        raise ValueError("one catalogue is a batch and the other is not")
    sep, code = check_match_args(max_sep, path, len(i1), len(i2))
    _B.require_gpu()
    s1, s2 = _MatchSide(cat1), _MatchSide(cat2)
    check_match_args(max_sep, path, s1.B, s2.B, s1.cap, s2.cap)
    B = s1.B
    m1 = torch.empty((B, s1.cap), dtype=torch.int32, device="cuda")
    m2 = torch.empty((B, s2.cap), dtype=torch.int32, device="cuda")
    sp = torch.empty((B, s1.cap), dtype=torch.float64, device="cuda")
    npairs = torch.empty((B,), dtype=torch.int32, device="cuda")
    st = torch.empty((B,), dtype=torch.int32, device="cuda")
    _B.check(_B.lib().bsgp_match_catalogs(*s1.args(), *s2.args(), B, sep, code, _B._ptr(m1),
                                          _B._ptr(m2), _B._ptr(sp), _B._ptr(npairs), _B._ptr(st),
                                          _B.current_stream()))
    m1h, m2h, sph, nph, sth = (t.cpu().numpy() for t in (m1, m2, sp, npairs, st))  # waits
    out = CatalogMatch([m1h[b, :s1.n[b]] for b in range(B)], [m2h[b, :s2.n[b]] for b in range(B)],
                       [sph[b, :s1.n[b]] for b in range(B)], sth, s1.labels, s2.labels, s1.batched)
    if not np.array_equal(np.atleast_1d(out.n_pairs), nph):
        raise _B.BsgpError(_B.BSGP_ERR_HIP, f"bsgp_match_catalogs reports {nph.tolist()} pairs, "
                           f"match1 holds {np.atleast_1d(out.n_pairs).tolist()}")
    if device_out:
        out.match1_dev, out.match2_dev, out.sep1_dev = m1, m2, sp
        out.n_pairs_dev, out.status_dev = npairs, st
    return out


def _one(match, cat1, cat2):
    if match.batched or getattr(cat1, "batched", False) or getattr(cat2, "batched", False) \
            or isinstance(cat1, list) or isinstance(cat2, list):
        raise ValueError("one image at a time: pass the images of a batch one by one")


def matched_columns(match, cat1, cat2, columns=None):
    """The joined table of a match, in the layout of the reference's published
    ``*_MATCHED.csv``: a dict of ``name_1`` for every column (the rows
    ``match.idx1`` of ``cat1``), then ``name_2`` (the rows ``match.idx2`` of
    ``cat2``), then ``Separation``.  ``columns``: the names (default: those of
    ``cat1.to_dict()`` / ``cat1.keys()`` that ``cat2`` has too).  Host only;
    the values are copied unchanged."""
    _one(match, cat1, cat2)
    if columns is None:
        names = [list(c.to_dict()) if isinstance(c, SourceCatalog) else list(c.keys())
                 for c in (cat1, cat2)]
        columns = [k for k in names[0] if k in names[1]]
    out = {}
    for tag, cat, idx in (("_1", cat1, match.idx1), ("_2", cat2, match.idx2)):
        for k in columns:
            out[k + tag] = np.asarray(getattr(cat[k], "value", cat[k]))[idx]
    out["Separation"] = np.asarray(match.separation)
    return out


def matched_metrics(orig, restored, max_sep=1.1, match=None):
    """The per-star comparison of a restored with an original catalogue -- what
    application_sgp_subdivisions.py:131-139 has commented out, because the two
    catalogues differ in length and order.  ``restored`` is matched as
    catalogue 1 and ``orig`` as catalogue 2, as in the reference's published
    tables (``match``: a :class:`CatalogMatch` made that way, instead of
    :func:`match_catalogs`).  Per pair, from the catalogues' columns on the
    host: ``flux_fractional_difference = 1 - restored.segment_flux /
    orig.segment_flux``, ``fwhm_ratio`` and ``ellipticity_ratio`` (restored over
    original), ``separation``, ``orig_label``, ``restored_label`` (``None``
    without a ``label`` column); ``median_flux_fractional_difference``,
    ``median_fwhm_ratio``, ``median_ellipticity_ratio`` (NaN without a pair);
    ``n_pairs``, ``n_orig``, ``n_restored``."""
    if match is None:
        match = match_catalogs(restored, orig, max_sep)
    _one(match, restored, orig)
    r, o = ({k: np.asarray(getattr(c[k], "value", c[k]), dtype=np.float64) for k in METRIC_COLUMNS}
            for c in (restored, orig))
    i, j = match.idx1, match.idx2
    with np.errstate(invalid="ignore", divide="ignore"):
        out = dict(flux_fractional_difference=1.0 - r["segment_flux"][i] / o["segment_flux"][j],
                   fwhm_ratio=r["fwhm"][i] / o["fwhm"][j],
                   ellipticity_ratio=r["ellipticity"][i] / o["ellipticity"][j])
    for k in tuple(out):
        out["median_" + k] = float(np.median(out[k])) if len(i) else float("nan")
    out.update(separation=np.asarray(match.separation), orig_label=match.labels2,
               restored_label=match.labels1, n_pairs=int(match.n_pairs),
               n_orig=len(o["segment_flux"]), n_restored=len(r["segment_flux"]))
    return out
