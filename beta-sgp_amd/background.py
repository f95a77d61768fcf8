"""Sky background of a field or a batch of images on the device.

The reference gets its background from ``utils.source_info``
(restoration/utils.py:235-239), which runs photutils'
``Background2D(data, box_size, filter_size=(3, 3),
bkg_estimator=MedianBackground())``: the per-pixel ``background`` map goes to
``sgp_betaDiv`` (application_sgp_subdivisions.py:62,85), ``background_median``
to the star-stamp application (application_sgp_star_stamps.py:63,83) and
``background_rms`` sets the detection threshold.  :class:`Background2D` here
keeps photutils' attribute names and computes all of it with one call of
``bsgp_background2d`` (include/bsgp.h; semantics in DESIGN §3.7): box
statistics by sigma clipping as ``astropy.stats.SigmaClip`` does it, the
excluded boxes filled from their nearest neighbours, a median filter over the
mesh and a cubic-spline zoom as ``scipy.ndimage.zoom(order=3, mode='reflect',
grid_mode=True)`` does it.
"""
import numpy as np

import _bsgp as _B


def _pair(v, name):
    """An int means a square; anything else must be a pair of ints."""
    if np.ndim(v) == 0:
        v = (v, v)
    v = tuple(v)
    if len(v) != 2 or any(int(s) != s for s in v):
        raise ValueError(f"{name} must be an int or a pair of ints, got {v!r}")
    return int(v[0]), int(v[1])


def check_args(shape, box_size, filter_size, sigma, maxiters, exclude_percentile, mask_shape=None):
    """The argument checks of Background2D (host only): returns (bh, bw), (fh, fw)."""
    if len(shape) not in (2, 3):
        raise ValueError(f"data must be [H, W] or [B, H, W], got shape {tuple(shape)}")
    bh, bw = _pair(box_size, "box_size")
    fh, fw = _pair(filter_size, "filter_size")
    if bh <= 0 or bw <= 0:
        raise ValueError(f"box_size must be positive, got {(bh, bw)}")
    if fh <= 0 or fw <= 0 or fh % 2 == 0 or fw % 2 == 0:
        raise ValueError(f"filter_size must be odd and positive, got {(fh, fw)}")
    if not sigma >= 0:
        raise ValueError(f"sigma must be >= 0, got {sigma}")
    if int(maxiters) != maxiters or maxiters < 0:
        raise ValueError(f"maxiters must be a non-negative int, got {maxiters}")
    if not 0 <= exclude_percentile <= 100:
        raise ValueError(f"exclude_percentile must be in [0, 100], got {exclude_percentile}")
    if mask_shape is not None and tuple(mask_shape) != tuple(shape) and \
            tuple(mask_shape) != tuple(shape[-2:]):
        raise ValueError(f"mask shape {tuple(mask_shape)} does not match data shape {tuple(shape)}")
    return (bh, bw), (fh, fw)


class Background2D:
    """``Background2D(data, box_size, filter_size=(3, 3), ...)`` on the device.

    ``data``: [H, W] or [B, H, W] (B images of one shape, each estimated on its
    own), numpy array or CUDA tensor, float32 or float64 (anything else is
    widened to float64 first).  ``mask``: boolean, True = ignore the pixel;
    data-shaped, or [H, W] for every image of a batch.  Non-finite pixels are
    ignored as well.  A box holds at most 4096 pixels.

    Attributes (numpy, or CUDA tensors with ``device_out=True``; a batch adds a
    leading B axis): ``background``, ``background_rms`` [H, W];
    ``background_mesh``, ``background_rms_mesh`` [ny, nx] (filled and
    median-filtered); ``background_median``, ``background_rms_median``.
    Beyond photutils: ``mesh_excluded`` (boxes left out and filled),
    ``mesh_npixels`` (pixels that survived clipping) and ``mesh_iterations``
    (clipping iterations run), each [ny, nx] on the host.

    Raises ``ValueError`` if every box of an image is excluded.
    """

    def __init__(self, data, box_size, filter_size=(3, 3), sigma=3.0, maxiters=10,
                 exclude_percentile=10.0, clip=True, mask=None, device_out=False):
        torch = _B.torch
        is_t = torch is not None and torch.is_tensor(data)
        shape = tuple(data.shape) if is_t else np.shape(data)
        m_is_t = mask is not None and torch is not None and torch.is_tensor(mask)
        mshape = None if mask is None else (tuple(mask.shape) if m_is_t else np.shape(mask))
        (bh, bw), (fh, fw) = check_args(shape, box_size, filter_size, sigma, maxiters,
                                        exclude_percentile, mshape)
        _B.require_gpu()
        if is_t:
            d = data if data.dtype in (torch.float32, torch.float64) else data.to(torch.float64)
            d = d.to("cuda").contiguous()
        else:
            d = np.asarray(data)
            if not (d.dtype.kind == "f" and d.dtype.itemsize in (4, 8)):
                d = d.astype(np.float64)
            d = torch.from_numpy(np.ascontiguousarray(d.astype(d.dtype.newbyteorder("=")))).to("cuda")
        batched = d.dim() == 3
        if not batched:
            d = d[None]
        B, H, W = d.shape
        m = None
        if mask is not None:
            m = mask if m_is_t else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
            m = (m != 0).to("cuda")
            m = m.expand(B, H, W) if m.dim() == 2 else m
            m = m.to(torch.uint8).contiguous()
        ny, nx = -(-H // bh), -(-W // bw)
        f64 = dict(dtype=torch.float64, device="cuda")
        bkg = torch.empty((B, H, W), **f64)
        rms = torch.empty((B, H, W), **f64)
        mesh = torch.empty((B, ny, nx), **f64)
        rmesh = torch.empty((B, ny, nx), **f64)
        med = torch.empty((B, 2), **f64)
        status = torch.empty((B, 1 + 3 * ny * nx), dtype=torch.int32, device="cuda")
        dtype = _B.BSGP_DTYPE_F32 if d.dtype == torch.float32 else _B.BSGP_DTYPE_F64
        _B.check(_B.lib().bsgp_background2d(
            _B._ptr(d), dtype, B, H, W, bh, bw, fh, fw, float(sigma), int(maxiters),
            float(exclude_percentile), int(bool(clip)), _B._ptr(m), _B._ptr(bkg), _B._ptr(rms),
            _B._ptr(mesh), _B._ptr(rmesh), _B._ptr(med), _B._ptr(status), _B.current_stream()))
        st = status.cpu().numpy()  # waits for the kernels
        empty = np.flatnonzero(st[:, 0] == 0)
        if len(empty):
            raise ValueError(f"image {int(empty[0])}: every box was excluded (more than "
                             f"{exclude_percentile} % of each box's pixels are masked, non-finite "
                             "or outside the image); raise exclude_percentile or change box_size")
        cells = st[:, 1:].reshape(B, 3, ny, nx)

        def pick(t, host=not device_out):
            t = t if batched else t[0]
            return t.cpu().numpy() if host else t

        self.box_size, self.filter_size = (bh, bw), (fh, fw)
        self.background, self.background_rms = pick(bkg), pick(rms)
        self.background_mesh, self.background_rms_mesh = pick(mesh), pick(rmesh)
        medh = med.cpu().numpy()
        self.background_median = medh[:, 0] if batched else float(medh[0, 0])
        self.background_rms_median = medh[:, 1] if batched else float(medh[0, 1])
        self.mesh_excluded = (cells[:, 0] if batched else cells[0, 0]).astype(bool)
        self.mesh_npixels = cells[:, 1] if batched else cells[0, 1]
        self.mesh_iterations = cells[:, 2] if batched else cells[0, 2]
