"""Finding and measuring the stars of a frame on the device: what the
reference leaves to DIAPL's ``sfind`` and ``fwhmm`` and to the star choice of
``getpsf`` (psf/psf_estimation.bash, psf/psf_steps_and_params.MD).  The defaults
are the published parameter files' (``sfind.par``, ``fwhmm.par``,
``getpsf.par``); the rule is DESIGN §3.15, F1 to F10, restated in numpy in
tests/starfind_ref.py.

    stars = find_stars(frame, fwhm=4.5, noise=bkg)     # a Background2D, a map or a number
    fwhm = stars.seeing()                              # fwhmm's role; call find_stars again
    sel, eligible, rank = select_psf_stars(stars)
    fit = fit_psf(frame, fwhm=fwhm, **stars.psf_inputs(sel))
    write_coo("frame.coo", stars)

Everything numerical runs in libbsgp's kernels (``bsgp_star_maps``,
``bsgp_star_peaks``, ``bsgp_star_measure``, ``bsgp_star_select``); there is no
CPU fallback."""
import warnings

import numpy as np

import _bsgp as _B

MAX_R, MAX_STARS = _B.BSGP_STARFIND_MAX_R, _B.BSGP_STARFIND_MAX
MAX_SKY = _B.BSGP_LOCALBKG_MAX
MAX_ANRAD = 1025.0  # anrad2 stays below it
BAD_FLUX, OFF_CENTRE = _B.BSGP_STARFIND_BAD_FLUX, _B.BSGP_STARFIND_OFF_CENTRE
FEW_SKY, SKY_OVER_CAP = _B.BSGP_STARFIND_FEW_SKY, _B.BSGP_STARFIND_SKY_OVER_CAP
REJECTED, OVER_CAP = _B.BSGP_STARFIND_REJECTED, _B.BSGP_STARFIND_OVER_CAP
# sfind.par / getpsf.par / fwhmm.par
APRAD, ANRAD1, ANRAD2, C_MIN, THRESH, DXY = 1.2, 20.0, 25.0, 0.4, 2.0, 1.0
PSFHW, MIN_FLUX, RAT_THRESH, FITRAD, NPSF_MAX = 15, 100.0, 0.2, 3.0, 100
# the sky's clipping (the local background's L4) and its smallest sample
SKY_SIGMA, SKY_MAXITERS, MIN_SKY = 3.0, 10, 10
FWHM_TO_SIGMA = 0.42466090014400953  # astropy's gaussian_fwhm_to_sigma
BKG_ALGS = {"mode": _B.BSGP_STARFIND_BKG_MODE, "median": _B.BSGP_STARFIND_BKG_MEDIAN,
            "mean": _B.BSGP_STARFIND_BKG_MEAN}
FCOLS = ("x", "y", "flux", "bkg", "peak", "corr", "amp", "fwhm")
ICOLS = ("ic", "ir", "nsat", "status")
COO_HEADER = "# x y approx_flux local_bkg_level num_saturated_pixels_in_aperture"


class StarCapWarning(UserWarning):
    """More candidates than ``max_stars``, or a sky annulus over the LDS cap."""


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def star_template(fwhm, aprad=APRAD):
    """F1, on the host: dict(R, rap, n, dy [n], dx [n], halfw [2R + 1] int32,
    t [n], tt).  The support is |dy|, |dx| <= R with dx^2 + dy^2 <= rap^2 in
    row-major order, t the Gaussian of ``fwhm`` on it minus its mean."""
    rap = aprad * fwhm
    R = int(np.floor(rap))
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    r2 = (dx * dx + dy * dy).astype(np.float64)
    inside = r2 <= rap * rap
    dy, dx, r2 = dy[inside], dx[inside], r2[inside]
    sigma = fwhm * FWHM_TO_SIGMA
    g = np.exp(-r2 / (2.0 * sigma * sigma))
    t = g - g.sum() / len(g)
    halfw = np.array([dx[dy == r].max() for r in range(-R, R + 1)], dtype=np.int32)
    return dict(R=R, rap=rap, n=len(t), dy=dy, dx=dx, halfw=halfw, t=t, tt=float(np.sum(t * t)))


def annulus_pixels(anrad1, anrad2):
    """Pixels of a sky annulus that lies inside the frame (geometry alone)."""
    box = int(np.floor(anrad2))
    d = np.arange(-box, box + 1, dtype=np.int64)
    d2 = (d[None, :] * d[None, :] + d[:, None] * d[:, None]).astype(np.float64)
    return int(np.count_nonzero((d2 >= anrad1 * anrad1) & (d2 <= anrad2 * anrad2)))


def check_find_args(image_shape, fwhm, noise_shape=(), mask_shape=None, sat_level=None,
                    c_min=C_MIN, aprad=APRAD, anrad1=ANRAD1, anrad2=ANRAD2, thresh=THRESH, dxy=DXY,
                    bkg_alg="mode", peak_hw=1, max_stars=None):
    """The argument checks of find_stars (host only; nothing touches the GPU).
    The image is [H, W] or [B, H, W]; ``noise`` a number (shape ()), one per
    frame [B], a map [H, W] shared by the frames or maps [B, H, W]; a mask has
    the image's shape.  ``fwhm`` and ``aprad`` are > 0 with
    R = floor(aprad * fwhm) at most ``MAX_R``; 0 <= anrad1 < anrad2 < 1025;
    ``peak_hw`` is an int in 0..3; ``max_stars`` an int in 1..``MAX_STARS``
    (default ``MAX_STARS``); ``bkg_alg`` one of 'mode', 'median', 'mean'.
    Returns a dict of the resolved values, among them ``annulus_pixels`` (of an
    annulus inside the frame) and ``sky_over_cap``: whether that is more than
    the ``MAX_SKY`` values a sky may hold (such stars get ``SKY_OVER_CAP``), and
    ``empty``: the frame is smaller than the support, no pixel is valid."""
    ishape = tuple(int(v) for v in image_shape)
    if len(ishape) not in (2, 3) or min(ishape) < 1:
        raise ValueError(f"image must be [H, W] or [B, H, W], got shape {ishape}")
    batched = len(ishape) == 3
    B, (H, W) = (ishape[0] if batched else 1), ishape[-2:]
    for nm, v in (("fwhm", fwhm), ("aprad", aprad)):
        if not _is_number(v) or not np.isfinite(v) or v <= 0:
            raise ValueError(f"{nm} must be a finite number > 0, got {v!r}")
    rap = float(aprad) * float(fwhm)
    R = int(np.floor(rap))
    if R > MAX_R:
        raise ValueError(f"aprad * fwhm = {rap:g}: the support reaches R = {R} pixels, at most "
                         f"MAX_R = {MAX_R}")
    for nm, v in (("c_min", c_min), ("thresh", thresh), ("dxy", dxy), ("anrad1", anrad1),
                  ("anrad2", anrad2)):
        if not _is_number(v) or not np.isfinite(v):
            raise ValueError(f"{nm} must be a finite number, got {v!r}")
    if not 0 <= anrad1 < anrad2:
        raise ValueError(f"the sky annulus needs 0 <= anrad1 < anrad2, got {anrad1!r}, {anrad2!r}")
    if anrad2 >= MAX_ANRAD:
        raise ValueError(f"anrad2 must be below {MAX_ANRAD:g}, got {anrad2!r}")
    if dxy < 0:
        raise ValueError(f"dxy must be >= 0, got {dxy!r}")
    if not _is_int(peak_hw) or not 0 <= peak_hw <= 3:
        raise ValueError(f"peak_hw must be an int in 0..3, got {peak_hw!r}")
    if max_stars is None:
        max_stars = MAX_STARS
    if not _is_int(max_stars) or not 1 <= max_stars <= MAX_STARS:
        raise ValueError(f"max_stars must be an int in 1..MAX_STARS = {MAX_STARS}, got {max_stars!r}")
    if bkg_alg not in BKG_ALGS:
        raise ValueError(f"bkg_alg must be one of {sorted(BKG_ALGS)}, got {bkg_alg!r}")
    if sat_level is not None and (not _is_number(sat_level) or np.isnan(sat_level)):
        raise ValueError(f"sat_level must be a number or None, got {sat_level!r}")
    if mask_shape is not None and tuple(mask_shape) != ishape:
        raise ValueError(f"mask shape {tuple(mask_shape)} does not match image shape {ishape}")
    nshape = tuple(int(v) for v in noise_shape)
    if nshape == ():
        noise_mode = "number"
    elif batched and nshape == (B,):
        noise_mode = "frame"
    elif nshape == (H, W) or nshape == ishape:
        noise_mode = "map"
    else:
        raise ValueError(f"noise shape {nshape}: a number, one per frame, or a map of the image's "
                         f"shape {ishape}")
    npix = annulus_pixels(float(anrad1), float(anrad2))
    return dict(batched=batched, B=B, H=H, W=W, fwhm=float(fwhm), aprad=float(aprad), rap=rap, R=R,
                c_min=float(c_min), thresh=float(thresh), dxy=float(dxy), anrad1=float(anrad1),
                anrad2=float(anrad2), peak_hw=int(peak_hw), max_stars=int(max_stars),
                bkg_alg=bkg_alg, noise_mode=noise_mode, annulus_pixels=npix,
                sky_over_cap=npix > MAX_SKY, empty=H < 2 * R + 1 or W < 2 * R + 1)


def check_select_args(hw=PSFHW, min_flux=MIN_FLUX, max_peak=None, rat_thresh=RAT_THRESH,
                      iso_radius=None, npsf_max=NPSF_MAX, fwhm=None):
    """The argument checks of select_psf_stars (host only)."""
    if not _is_int(hw) or hw < 0:
        raise ValueError(f"hw must be an int >= 0, got {hw!r}")
    if not _is_int(npsf_max) or npsf_max < 0:
        raise ValueError(f"npsf_max must be an int >= 0, got {npsf_max!r}")
    if iso_radius is None:
        if fwhm is None:
            raise ValueError("iso_radius defaults to 3 fwhm: give one of them")
        iso_radius = FITRAD * fwhm
    for nm, v in (("min_flux", min_flux), ("rat_thresh", rat_thresh), ("iso_radius", iso_radius)):
        if not _is_number(v) or np.isnan(v):
            raise ValueError(f"{nm} must be a number, got {v!r}")
    if iso_radius < 0:
        raise ValueError(f"iso_radius must be >= 0, got {iso_radius!r}")
    if max_peak is not None and (not _is_number(max_peak) or np.isnan(max_peak)):
        raise ValueError(f"max_peak must be a number or None, got {max_peak!r}")
    return dict(hw=int(hw), min_flux=float(min_flux), max_peak=max_peak,
                rat_thresh=float(rat_thresh), iso_radius=float(iso_radius), npsf_max=int(npsf_max))


class StarList:
    """The stars of one frame (result of :func:`find_stars`), numbered in
    raster order of their peak pixel; rows are never dropped or renumbered.

    Columns, arrays over the ``n`` stars (CUDA tensors with ``device_out``):
    ``x``, ``y`` (0-based centroid, x the column; also ``xcentroid``,
    ``ycentroid``), ``flux`` (aperture sum minus sky), ``bkg`` (sky), ``peak``
    (brightest pixel minus sky), ``corr``, ``amp`` (the maps at the peak
    pixel), ``fwhm`` (from the second moments), ``ic``, ``ir`` (peak pixel),
    ``nsat``, ``status`` (``BAD_FLUX | OFF_CENTRE | FEW_SKY | SKY_OVER_CAP``)
    and ``kept`` (no rejecting bit).  ``frame_status`` is 0 or ``OVER_CAP``.
    ``fcols`` [cap, 8] and ``icols`` [cap, 4] are the device tensors;
    ``corr_map`` / ``amp_map`` exist with ``return_maps``."""

    def __init__(self, fcols, icols, n, shape, fwhm, frame_status=0, device_out=False, host=None):
        self.fcols, self.icols, self.n = fcols, icols, int(n)
        self.shape, self.template_fwhm, self.frame_status = tuple(shape), fwhm, int(frame_status)
        self.device_out = device_out
        if host is None:
            host = _B.to_host(dict(f=fcols, i=icols))
        self._f, self._i = host["f"][:self.n], host["i"][:self.n]
        src_f, src_i = (fcols, icols) if device_out else (self._f, self._i)
        for k, name in enumerate(FCOLS):
            setattr(self, name, src_f[:self.n, k])
        for k, name in enumerate(ICOLS):
            setattr(self, name, src_i[:self.n, k])
        self.xcentroid, self.ycentroid = self.x, self.y
        self.kept = (self.status & REJECTED) == 0

    @classmethod
    def from_columns(cls, x, y, flux, shape, fwhm=None, bkg=None, peak=None, nsat=None,
                     status=None, device_out=False):
        """A StarList from host columns (a catalogue from elsewhere, a .coo
        file): what :func:`select_psf_stars` and ``psf_inputs`` need."""
        _B.require_gpu()
        torch = _B.torch
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        n = len(x)
        f = np.full((max(1, n), 8), np.nan)
        i = np.zeros((max(1, n), 4), dtype=np.int32)
        f[:n, 0], f[:n, 1], f[:n, 2] = x, np.asarray(y, dtype=np.float64), np.asarray(flux, dtype=np.float64)
        f[:n, 3] = 0.0 if bkg is None else np.asarray(bkg, dtype=np.float64)
        f[:n, 4] = f[:n, 2] if peak is None else np.asarray(peak, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            i[:n, 0], i[:n, 1] = np.floor(f[:n, 0] + 0.5), np.floor(f[:n, 1] + 0.5)
        i[:n, 2] = 0 if nsat is None else np.asarray(nsat)
        i[:n, 3] = 0 if status is None else np.asarray(status)
        return cls(torch.from_numpy(f).to("cuda"), torch.from_numpy(i).to("cuda"), n, shape, fwhm,
                   device_out=device_out, host=dict(f=f, i=i))

    def __len__(self):
        return self.n

    def keys(self):
        return list(FCOLS + ICOLS) + ["xcentroid", "ycentroid", "kept"]

    def __getitem__(self, name):
        if name not in self.keys():
            raise KeyError(name)
        v = getattr(self, name)
        return v.cpu().numpy() if self.device_out else v

    def table(self, kept_only=True):
        """[m, 5] float64: the .coo columns x, y, approx_flux, local_bkg_level,
        num_saturated_pixels_in_aperture of the kept stars (or of all)."""
        t = np.column_stack([self._f[:, 0], self._f[:, 1], self._f[:, 2], self._f[:, 3],
                             self._i[:, 2].astype(np.float64)])
        return t[(self._i[:, 3] & REJECTED) == 0] if kept_only else t

    def seeing(self, min_fwhm=2.6, max_fwhm=10.0, min_peak=500.0, max_peak=2e4, margin=5):
        """fwhmm's role: the median ``fwhm`` of the kept stars inside
        fwhmm.par's limits (MIN_FWHM, MAX_FWHM, MIN_PEAK, MAX_PEAK, MARGIN
        pixels from the frame's edge); NaN when there is none.  Call
        find_stars with a guess, take seeing(), call again.  Host columns."""
        H, W = self.shape
        f, st = self._f, self._i[:, 3]
        with np.errstate(invalid="ignore"):
            ok = ((st & REJECTED) == 0) & (f[:, 7] >= min_fwhm) & (f[:, 7] <= max_fwhm) & \
                (f[:, 4] >= min_peak) & (f[:, 4] <= max_peak) & \
                (f[:, 0] >= margin) & (f[:, 0] <= W - 1 - margin) & \
                (f[:, 1] >= margin) & (f[:, 1] <= H - 1 - margin)
        return float(np.median(f[ok, 7])) if ok.any() else float("nan")

    def psf_inputs(self, sel):
        """``dict(positions=[m, 2], flux=[m], background=[m])`` of the stars
        ``sel``: ``fit_psf(image, fwhm=f, **stars.psf_inputs(sel))``."""
        sel = np.asarray(sel, dtype=np.int64).reshape(-1)
        return dict(positions=self._f[sel, :2].copy(), flux=self._f[sel, 2].copy(),
                    background=self._f[sel, 3].copy())


class StarLists(list):
    """The :class:`StarList` of every frame of a batch, with the batch's device
    tensors ``fcols`` [B, cap, 8], ``icols`` [B, cap, 4], ``n`` [B] and
    ``frame_status`` [B] (host arrays)."""


def _dtype(d):
    return _B.BSGP_DTYPE_F32 if d.dtype == _B.torch.float32 else _B.BSGP_DTYPE_F64


def _template_dev(tp):
    torch = _B.torch
    t = torch.from_numpy(np.ascontiguousarray(tp["t"], dtype=np.float64)).to("cuda")
    return t, np.ascontiguousarray(tp["halfw"], dtype=np.int32)


def _mask_dev(mask, B, H, W):
    torch = _B.torch
    if mask is None:
        return None
    m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask) != 0)
    return (m != 0).to(torch.uint8).to("cuda").contiguous().reshape(B, H, W)


def _noise_dev(noise, c):
    """float64 CUDA tensor [B] or [B, H, W] and whether it is a map."""
    torch = _B.torch
    B, H, W = c["B"], c["H"], c["W"]
    if c["noise_mode"] == "number":
        return torch.full((B,), float(noise), dtype=torch.float64, device="cuda"), 0
    t = noise if torch.is_tensor(noise) else torch.from_numpy(
        np.ascontiguousarray(noise, dtype=np.float64))
    t = t.to("cuda").to(torch.float64)
    if c["noise_mode"] == "frame":
        return t.contiguous(), 0
    return t.expand(B, H, W).contiguous() if t.dim() == 2 else t.contiguous(), 1


def _maps_dev(d, mask, t, halfw, R, tt):
    """bsgp_star_maps: (corr, amp) [B, H, W].  Asynchronous."""
    torch = _B.torch
    B, H, W = d.shape
    corr, amp = torch.empty((B, H, W), dtype=torch.float64, device="cuda"), \
        torch.empty((B, H, W), dtype=torch.float64, device="cuda")
    _B.check(_B.lib().bsgp_star_maps(_B._ptr(d), _dtype(d), B, H, W, _B._ptr(mask), _B._ptr(t),
                                     halfw.ctypes.data, R, tt, _B._ptr(corr), _B._ptr(amp),
                                     _B.current_stream()))
    return corr, amp


def _peaks_dev(d, corr, amp, t, halfw, tt, nz, nz_map, c):
    """bsgp_star_peaks: (peaks [B, cap, 2], n [B], frame status [B]).  Asynchronous."""
    torch = _B.torch
    B, H, W = d.shape
    cap = c["max_stars"]
    i32 = dict(dtype=torch.int32, device="cuda")
    peaks, nd, fst = torch.empty((B, cap, 2), **i32), torch.empty((B,), **i32), \
        torch.empty((B,), **i32)
    _B.check(_B.lib().bsgp_star_peaks(_B._ptr(d), _dtype(d), B, H, W, _B._ptr(corr), _B._ptr(amp),
                                      _B._ptr(t), halfw.ctypes.data, c["R"], tt, _B._ptr(nz),
                                      nz_map, c["c_min"], c["thresh"], c["peak_hw"], cap,
                                      _B._ptr(peaks), _B._ptr(nd), _B._ptr(fst),
                                      _B.current_stream()))
    return peaks, nd, fst


def _measure_dev(d, m, corr, amp, halfw, peaks, nd, c, sat_level):
    """bsgp_star_measure on peaks [B, rows, 2]: (fcols [B, rows, 8], icols
    [B, rows, 4]).  Asynchronous."""
    torch = _B.torch
    B, H, W = d.shape
    rows = peaks.shape[1]
    fcols = torch.empty((B, rows, 8), dtype=torch.float64, device="cuda")
    icols = torch.empty((B, rows, 4), dtype=torch.int32, device="cuda")
    _B.check(_B.lib().bsgp_star_measure(
        _B._ptr(d), _dtype(d), B, H, W, _B._ptr(m), _B._ptr(corr), _B._ptr(amp),
        halfw.ctypes.data, c["R"], _B._ptr(peaks), _B._ptr(nd), rows, c["anrad1"], c["anrad2"],
        BKG_ALGS[c["bkg_alg"]], SKY_SIGMA, SKY_MAXITERS, MIN_SKY, int(sat_level is not None),
        0.0 if sat_level is None else float(sat_level), c["dxy"], _B._ptr(fcols), _B._ptr(icols),
        _B.current_stream()))
    return fcols, icols


def _select_dev(fcols, icols, nd, shape, c):
    """bsgp_star_select on [B, rows, .] columns: (eligible, rank, selected)
    [B, rows] int32.  Asynchronous."""
    torch = _B.torch
    B, rows = fcols.shape[0], fcols.shape[1]
    el, rk, se = (torch.empty((B, rows), dtype=torch.int32, device="cuda") for _ in range(3))
    _B.check(_B.lib().bsgp_star_select(
        _B._ptr(fcols), _B._ptr(icols), _B._ptr(nd), B, rows, shape[0], shape[1], c["hw"],
        c["min_flux"], int(c["max_peak"] is not None),
        0.0 if c["max_peak"] is None else float(c["max_peak"]), c["rat_thresh"], c["iso_radius"],
        c["npsf_max"], _B._ptr(el), _B._ptr(rk), _B._ptr(se), _B.current_stream()))
    return el, rk, se


def find_stars(image, fwhm, noise, mask=None, sat_level=None, c_min=C_MIN, aprad=APRAD,
               anrad1=ANRAD1, anrad2=ANRAD2, thresh=THRESH, dxy=DXY, bkg_alg="mode", peak_hw=1,
               max_stars=None, return_maps=False, device_out=False):
    """Find and measure the stars of a frame [H, W] or of every frame of a
    batch [B, H, W] (float32 or float64), on the device: DIAPL's ``sfind``
    (the defaults are sfind.par's).

    A zero-mean Gaussian template of ``fwhm`` on the aperture of radius
    ``aprad * fwhm`` is correlated with the frame; a pixel is a candidate when
    its correlation is at least ``c_min``, the matched filter's significance
    is at least ``thresh`` times ``noise`` (a number, one per frame, a map, or
    a :class:`background.Background2D`, whose ``background_rms`` is used) and
    its fitted amplitude is the maximum of the ``(2 peak_hw + 1)^2`` window.
    Every candidate gets a sky from the annulus ``anrad1 .. anrad2``
    (``bkg_alg``: 'mode', 'median' or 'mean' of the sigma-clipped values), the
    aperture's flux, centroid, moment FWHM and peak, the saturated pixels
    (``>= sat_level``) and the rejection bits; pixels that are not finite or
    masked (``mask`` nonzero) invalidate the apertures they fall in and are
    left out of a sky.  At most ``max_stars`` candidates are kept.

    Returns a :class:`StarList`, for a batch a :class:`StarLists` of them."""
    torch = _B.torch
    rms = getattr(noise, "background_rms", None)
    if rms is not None:
        noise = rms
    nshape = () if np.ndim(noise) == 0 and not (torch is not None and torch.is_tensor(noise)) \
        else tuple(noise.shape) if hasattr(noise, "shape") else np.shape(noise)
    c = check_find_args(tuple(image.shape), fwhm, nshape, None if mask is None else tuple(mask.shape),
                        sat_level, c_min, aprad, anrad1, anrad2, thresh, dxy, bkg_alg, peak_hw,
                        max_stars)
    if c["noise_mode"] == "number" and not _is_number(noise):
        noise = float(np.asarray(noise))
    _B.require_gpu()
    if c["sky_over_cap"]:
        warnings.warn(f"find_stars: the sky annulus holds {c['annulus_pixels']} pixels, a sky at "
                      f"most {MAX_SKY} values: stars with more get SKY_OVER_CAP and no sky",
                      StarCapWarning, stacklevel=2)
    import segmentation as _S
    d, batched = _S._to_dev(image)
    B, H, W, R, cap = c["B"], c["H"], c["W"], c["R"], c["max_stars"]
    tp = star_template(c["fwhm"], c["aprad"])
    t, halfw = _template_dev(tp)
    m = _mask_dev(mask, B, H, W)
    nz, nz_map = _noise_dev(noise, c)
    corr, amp = _maps_dev(d, m, t, halfw, R, tp["tt"])
    peaks, nd, fst = _peaks_dev(d, corr, amp, t, halfw, tp["tt"], nz, nz_map, c)
    h = _B.to_host(dict(n=nd, st=fst))  # waits: the rows to measure
    n, frame_status = h["n"], h["st"]
    over = np.flatnonzero(frame_status & OVER_CAP)
    if len(over):
        warnings.warn(f"find_stars: frame(s) {over.tolist()} hold more than max_stars = {cap} "
                      f"candidates: the first {cap} in raster order are kept", StarCapWarning,
                      stacklevel=2)
    rows = max(1, int(n.max()))
    peaks = peaks[:, :rows].contiguous()
    fcols, icols = _measure_dev(d, m, corr, amp, halfw, peaks, nd, c, sat_level)
    host = _B.to_host(dict(f=fcols, i=icols))
    out = StarLists()
    for b in range(B):
        s = StarList(fcols[b], icols[b], n[b], (H, W), c["fwhm"], frame_status[b], device_out,
                     host=dict(f=host["f"][b], i=host["i"][b]))
        if return_maps:
            s.corr_map = corr[b] if device_out else corr[b].cpu().numpy()
            s.amp_map = amp[b] if device_out else amp[b].cpu().numpy()
        out.append(s)
    if not batched:
        return out[0]
    out.fcols, out.icols, out.n, out.frame_status = fcols, icols, n, frame_status
    return out


def select_psf_stars(stars, hw=PSFHW, min_flux=MIN_FLUX, max_peak=None, rat_thresh=RAT_THRESH,
                     iso_radius=None, npsf_max=NPSF_MAX):
    """Choose the PSF stars of a :class:`StarList` on the device
    (``bsgp_star_select``; the defaults are getpsf.par's): a
    kept star is eligible when ``flux >= min_flux``, ``nsat == 0``,
    ``peak <= max_peak`` (if given), its ``(2 hw + 1)^2`` box lies inside the
    frame and no other kept star with at least ``rat_thresh`` of its flux lies
    within ``iso_radius`` (default 3 fwhm); the ``npsf_max`` brightest eligible
    stars are selected.  Returns ``(sel, eligible, rank)``: the selected
    indices in rank order (brightest first), and per star whether it is
    eligible and its rank among the eligible (-1 otherwise)."""
    c = check_select_args(hw, min_flux, max_peak, rat_thresh, iso_radius, npsf_max,
                          stars.template_fwhm)
    _B.require_gpu()
    torch = _B.torch
    nd = torch.full((1,), stars.n, dtype=torch.int32, device="cuda")
    el, rk, se = _select_dev(stars.fcols.contiguous()[None], stars.icols.contiguous()[None], nd,
                             stars.shape, c)
    h = _B.to_host(dict(el=el, rk=rk, se=se))
    n = stars.n
    eligible, rank, selected = h["el"][0, :n] != 0, h["rk"][0, :n], h["se"][0, :n] != 0
    sel = np.flatnonzero(selected)
    return sel[np.argsort(rank[sel], kind="stable")], eligible, rank


def write_coo(path, stars, index_base=0):
    """Write the kept stars as a .coo file: three header lines, then one row
    per star of five whitespace-separated columns x y approx_flux
    local_bkg_level num_saturated_pixels_in_aperture, which the application
    reads with ``numpy.loadtxt(path, skiprows=3)``.  ``stars``: a
    :class:`StarList` or an array [m, 5].  ``index_base`` is added to x and y
    (1 for a reader that counts pixels from 1)."""
    t = stars.table() if hasattr(stars, "table") else np.asarray(stars, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != 5:
        raise ValueError(f"a star table is [m, 5], got shape {t.shape}")
    with open(path, "w") as f:
        f.write(f"# stars: {len(t)}  index_base: {int(index_base)}\n")
        f.write("# found by beta-sgp_amd starfind.find_stars\n")
        f.write(COO_HEADER + "\n")
        for x, y, fl, bg, ns in t:
            f.write(f"{float(x + index_base)!r} {float(y + index_base)!r} {float(fl)!r} "
                    f"{float(bg)!r} {int(ns)}\n")


def read_coo(path, index_base=0):
    """The rows of a .coo file as [m, 5] float64 (three header lines skipped);
    ``index_base`` is subtracted from x and y."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # an empty file
        t = np.loadtxt(path, skiprows=3, ndmin=2, comments=None)
    t = t.reshape(-1, 5).astype(np.float64)
    t[:, :2] -= index_base
    return t
