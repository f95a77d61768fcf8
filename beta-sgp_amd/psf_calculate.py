"""DIAPL PSF model on the device: drop-in for psf/psf_calculate.py's ``PSF``
(SURVEY §8f row 4).

Same attributes and methods as the reference class (psf_calculate.py:9-165);
the stamps are computed by ``bsgp_psf_stamps`` on the GPU.  Two additions
serve the subdivision pipeline:

  psf.stamps(xy, normalize=True, device_out=False)
      one stamp per field position (x, y) through the model's spatial
      expansion (what init_psf, :140-165, sets out to do), as [n, S, S];
  psf.local_coeffs(x, y)
      the local coefficient vector at (x, y) — init_psf's result (the
      reference's version raises TypeError and returns nothing).

Stamps are (2hw+1)^2 with pixel (r, c) = calc_psf_pix(x = c - hw, y = r - hw),
exactly get_psf_mat's 31x31 layout for the hw = 15 of DIAPL's PSFHW.

The coefficient file itself the reference gets from DIAPL's ``getpsf``
(psf/psf_estimation.bash, psf/psf_steps_and_params.MD).  ``fit_psf`` fits the
coefficients to the stars of a frame on the device instead:
``PSF.from_values`` builds a model without a file, ``PSF.write`` writes the
file ``PSF(path)`` reads.
"""
import warnings

import numpy as np

import _bsgp as _B


class PSF:
    def __init__(self, txt_file):
        """Read a DIAPL coefficient file (psf_calculate.py:10-47)."""
        self.ldeg = 2
        self.sdeg = 1
        with open(txt_file) as f:
            data = [float(l.rstrip("\n")) for l in f]
        self.hw = int(data[0])
        self.ndeg_spat = int(data[1])
        self.ndeg_local = int(data[2])
        self.ngauss = int(data[3])
        self.recenter = data[4]
        self.cos = data[5]
        self.sin = data[6]
        self.ax = data[7]
        self.ay = data[8]
        self.sigma_inc = data[9]
        self.sigma_mscale = data[10]
        self.fitrad = data[11]
        self.x_orig = data[12]
        self.y_orig = data[13]
        self.vec_coeffs = data[14:]
        self.ntot = self.ngauss * (self.ndeg_local + 1) * (self.ndeg_local + 2) / 2
        self.ntot *= (self.ndeg_spat + 1) * (self.ndeg_spat + 2) / 2

    @classmethod
    def from_values(cls, hw, ngauss, ldeg, sdeg, cos, sin, ax, ay, sigma_inc, x_orig, y_orig,
                    coeffs, recenter=0.0, sigma_mscale=0.0, fitrad=0.0):
        """A model from its values, without a file: the 14 header values of a
        coefficient file (``ndeg_local = ldeg``, ``ndeg_spat = sdeg``) and the
        ``ngauss (ldeg+1)(ldeg+2)/2 * (sdeg+1)(sdeg+2)/2`` coefficients, spatial
        term by spatial term.  Unlike a file-built model, which always
        evaluates with ldeg = 2 and sdeg = 1 as the reference does, this one
        evaluates with the degrees given."""
        hw, ngauss, ldeg, sdeg = int(hw), int(ngauss), int(ldeg), int(sdeg)
        if hw < 0 or ngauss < 1 or ldeg < 0 or sdeg < 0:
            raise ValueError("hw, ldeg and sdeg must be >= 0 and ngauss >= 1")
        c = [float(v) for v in np.asarray(coeffs, dtype=np.float64).reshape(-1)]
        need = ngauss * (ldeg + 1) * (ldeg + 2) // 2 * ((sdeg + 1) * (sdeg + 2) // 2)
        if len(c) != need:
            raise ValueError(f"{len(c)} coefficients given, the degrees need {need}")
        self = cls.__new__(cls)
        self.ldeg, self.sdeg = ldeg, sdeg
        self.hw, self.ndeg_spat, self.ndeg_local, self.ngauss = hw, sdeg, ldeg, ngauss
        self.recenter = float(recenter)
        self.cos, self.sin, self.ax, self.ay = float(cos), float(sin), float(ax), float(ay)
        self.sigma_inc, self.sigma_mscale = float(sigma_inc), float(sigma_mscale)
        self.fitrad = float(fitrad)
        self.x_orig, self.y_orig = float(x_orig), float(y_orig)
        self.vec_coeffs = c
        self.ntot = float(need)
        return self

    def write(self, path):
        """Write the model as a coefficient file: the 14 header values and the
        coefficients, one per line, each float as its ``repr`` (which reads
        back to the same float64).  ``PSF(path)`` reads it; that constructor
        evaluates with ldeg = 2 and sdeg = 1 whatever the header says, so
        only a model of those degrees evaluates the same after a round trip."""
        head = [self.hw, self.ndeg_spat, self.ndeg_local, self.ngauss, self.recenter, self.cos,
                self.sin, self.ax, self.ay, self.sigma_inc, self.sigma_mscale, self.fitrad,
                self.x_orig, self.y_orig]
        with open(path, "w") as f:
            for v in head + list(self.vec_coeffs):
                f.write(repr(int(v)) if isinstance(v, (int, np.integer)) else repr(float(v)))
                f.write("\n")

    @property
    def coeffs(self):
        return self.vec_coeffs

    @property
    def ncomp(self):
        return self.ngauss * (self.ldeg + 1) * (self.ldeg + 2) // 2

    # ----------------------------------------------------------- device
    def _model(self, hw=None):
        c = np.ascontiguousarray(self.vec_coeffs, dtype=np.float64)
        m = _B.PsfModel(hw=self.hw if hw is None else hw, ngauss=self.ngauss, ldeg=self.ldeg,
                        sdeg=self.sdeg, cos=self.cos, sin=self.sin, ax=self.ax, ay=self.ay,
                        sigma_inc=self.sigma_inc, x_orig=self.x_orig, y_orig=self.y_orig,
                        coeffs=c.ctypes.data, ncoef=len(c))
        return m, c

    def _stamps(self, xy, n, normalize, hw=None):
        _B.require_gpu()
        torch = _B.torch
        m, keep = self._model(hw)
        S = 2 * m.hw + 1
        out = torch.empty((n, S, S), dtype=torch.float64, device="cuda")
        _B.check(_B.lib().bsgp_psf_stamps(_B.ctypes.byref(m), _B._ptr(xy) if xy is not None else None,
                                          n, int(xy is not None), int(bool(normalize)),
                                          _B._ptr(out), _B.current_stream()))
        del keep  # the coefficients are copied into the kernel arguments at launch
        return out

    def stamps(self, xy, normalize=True, device_out=False):
        """Stamps at field positions xy [n, 2] ((x, y) pairs): the local
        coefficients come from the spatial expansion about (x_orig, y_orig)."""
        torch = _B.torch
        _B.require_gpu()
        xy_d = xy.to(dtype=torch.float64).contiguous() if torch.is_tensor(xy) else \
            _B.to_dev(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
        out = self._stamps(xy_d, xy_d.shape[0], normalize)
        out._keep = xy_d
        if device_out:
            return out
        return out.cpu().numpy()

    def local_coeffs(self, x, y):
        """init_psf (:140-165): local coefficients at field position (x, y)."""
        ncomp = self.ncomp
        loc = [0.0] * ncomp
        itot = 0
        a1 = 1.0
        for m in range(self.sdeg + 1):
            a2 = 1.0
            for _ in range(self.sdeg - m + 1):
                for icomp in range(ncomp):
                    loc[icomp] += self.vec_coeffs[itot] * a1 * a2
                    itot += 1
                a2 *= y - self.y_orig
            a1 *= x - self.x_orig
        return loc

    def init_psf(self, xpsf, ypsf):
        """The reference's init_psf, returning the local coefficient vector."""
        return self.local_coeffs(xpsf, ypsf)

    # ------------------------------------------------------ reference API
    def calc_psf_pix(self, coeffs, x, y):
        """PSF value at integer pixel offset (x, y) (psf_calculate.py:52-87).
        As in the reference, the value uses the model's own coefficients
        (``coeffs`` is not read there either)."""
        if int(x) != x or int(y) != y:
            raise ValueError("calc_psf_pix evaluates integer pixel offsets")
        hw = max(abs(int(x)), abs(int(y)))
        st = self._stamps(None, 1, False, hw=hw)[0]
        return float(st[int(y) + hw, int(x) + hw])

    def get_psf_mat(self):
        """(2hw+1)^2 stamp at the expansion origin (psf_calculate.py:89-107)."""
        self.psf_mat = self._stamps(None, 1, False)[0].cpu().numpy()
        return self.psf_mat

    def show_psf_mat(self):
        import matplotlib.pyplot as plt  # display only (psf_calculate.py:109-114)
        plt.matshow(self.get_psf_mat(), origin='lower')
        plt.colorbar()
        plt.show()

    def check_symmetric(self, coeffs, rtol=1e-05, atol=1e-08):
        return np.allclose(coeffs, coeffs.T, rtol=rtol, atol=atol)

    def normalize_psf_mat(self):
        """Stamp divided by its sum (psf_calculate.py:129-137)."""
        self.get_psf_mat()
        return self._stamps(None, 1, True)[0].cpu().numpy()


# ---- fitting the model to a frame's stars (bsgp_psf_fit_*) ----
FIT_MAX_COEF, FIT_MAX_STARS = _B.BSGP_PSFFIT_MAX_COEF, _B.BSGP_PSFFIT_MAX_STARS
SIGMA_INC = 0.548  # getpsf.par


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def check_fit_args(image_shape, positions_shape, hw=15, ngauss=2, ldeg=2, sdeg=1, fwhm=None,
                   shape=None, sigma_inc=SIGMA_INC, fitrad=None, niter=0, nsig=2.0, min_stars=None,
                   origin=None, counts=None, mask_shape=None, flux_shape=None, weights_shape=None,
                   background_shape=None, sat_level=None):
    """The argument checks of fit_psf (host only; nothing touches the GPU).
    The image is [H, W] with positions [n, 2], or [B, H, W] with positions
    [B, n, 2] and (optionally) ``counts`` [B], each in 0..n; n is at most
    ``FIT_MAX_STARS``.  ``hw`` is an int in 1..255 (the box is 2 hw + 1 wide,
    always odd), the degrees are ints >= 0 and ``ngauss`` >= 1 with at most
    ``FIT_MAX_COEF`` coefficients in all; exactly one of ``fwhm`` (> 0) and
    ``shape`` = (cos, sin, ax, ay) is given; ``fitrad`` (default hw) is > 0.
    A mask has the image's shape; flux and weights have the positions' shape
    without its last axis; a background is a number, per star or a map.
    Returns a dict of the resolved values."""
    ishape = tuple(int(v) for v in image_shape)
    if len(ishape) not in (2, 3) or min(ishape) < 1:
        raise ValueError(f"image must be [H, W] or [B, H, W], got shape {ishape}")
    batched = len(ishape) == 3
    pshape = tuple(int(v) for v in positions_shape)
    if len(pshape) != len(ishape) or pshape[-1] != 2 or (batched and pshape[0] != ishape[0]):
        raise ValueError(f"positions must be [n, 2] in (x, y) for an image [H, W] and [B, n, 2] for "
                         f"a batch, got shape {pshape} beside image shape {ishape}")
    n = pshape[-2]
    if n > FIT_MAX_STARS:
        raise ValueError(f"{n} stars: a frame holds at most FIT_MAX_STARS = {FIT_MAX_STARS}")
    B = ishape[0] if batched else 1
    if counts is None:
        cnt = np.full(B, n, dtype=np.int32)
    else:
        if not batched:
            raise ValueError("counts goes with a batch [B, H, W]")
        cnt = np.asarray(counts)
        if cnt.shape != (B,) or cnt.dtype.kind not in "iu":
            raise ValueError(f"counts must be {B} ints, one per frame")
        if cnt.min() < 0 or cnt.max() > n:
            raise ValueError(f"counts must lie in 0..{n}, the positions each frame has")
        cnt = cnt.astype(np.int32)
    if not _is_int(hw) or hw < 1 or hw > 255:
        raise ValueError(f"hw must be an int in 1..255 (the fit box is 2 hw + 1 wide), got {hw!r}")
    for nm, v, lo in (("ngauss", ngauss, 1), ("ldeg", ldeg, 0), ("sdeg", sdeg, 0)):
        if not _is_int(v) or v < lo:
            raise ValueError(f"{nm} must be an int >= {lo}, got {v!r}")
    ncomp = int(ngauss) * (int(ldeg) + 1) * (int(ldeg) + 2) // 2
    nterm = (int(sdeg) + 1) * (int(sdeg) + 2) // 2
    if ncomp * nterm > FIT_MAX_COEF:
        raise ValueError(f"ngauss = {ngauss}, ldeg = {ldeg}, sdeg = {sdeg}: {ncomp * nterm} "
                         f"coefficients, a fit holds at most FIT_MAX_COEF = {FIT_MAX_COEF}")
    if (fwhm is None) == (shape is None):
        raise ValueError("give exactly one of fwhm and shape=(cos, sin, ax, ay)")
    if fwhm is not None:
        if not _is_number(fwhm) or not np.isfinite(fwhm) or fwhm <= 0:
            raise ValueError(f"fwhm must be a finite number > 0, got {fwhm!r}")
        a = -4.0 * np.log(2.0) / (float(fwhm) * float(fwhm))
        shp = (1.0, 0.0, a, a)
    else:
        shp = tuple(shape) if np.ndim(shape) == 1 else ()
        if len(shp) != 4 or not all(_is_number(v) and np.isfinite(v) for v in shp):
            raise ValueError(f"shape must be four finite numbers (cos, sin, ax, ay), got {shape!r}")
        shp = tuple(float(v) for v in shp)
    if not _is_number(sigma_inc) or not np.isfinite(sigma_inc):
        raise ValueError(f"sigma_inc must be a finite number, got {sigma_inc!r}")
    if fitrad is None:
        fitrad = float(hw)
    if not _is_number(fitrad) or not fitrad > 0:
        raise ValueError(f"fitrad must be a number > 0, got {fitrad!r}")
    if not _is_int(niter) or niter < 0:
        raise ValueError(f"niter must be an int >= 0, got {niter!r}")
    if not _is_number(nsig) or np.isnan(nsig):
        raise ValueError(f"nsig must be a number, got {nsig!r}")
    if min_stars is None:
        min_stars = 0
    if not _is_int(min_stars) or min_stars < 0:
        raise ValueError(f"min_stars must be an int >= 0, got {min_stars!r}")
    if origin is None:
        origin = (ishape[-1] / 2, ishape[-2] / 2)
    org = tuple(origin) if np.ndim(origin) == 1 else ()
    if len(org) != 2 or not all(_is_number(v) and np.isfinite(v) for v in org):
        raise ValueError(f"origin must be two finite numbers (x, y), got {origin!r}")
    if sat_level is not None and (not _is_number(sat_level) or np.isnan(sat_level)):
        raise ValueError(f"sat_level must be a number or None, got {sat_level!r}")
    if mask_shape is not None and tuple(mask_shape) != ishape:
        raise ValueError(f"mask shape {tuple(mask_shape)} does not match image shape {ishape}")
    per_star = pshape[:-1]
    for nm, sh in (("flux", flux_shape), ("weights", weights_shape)):
        if sh is not None and tuple(sh) != per_star:
            raise ValueError(f"{nm} shape {tuple(sh)}: one value per star is {per_star}")
    sky_mode = 0
    if background_shape is not None and tuple(background_shape) != ():
        if tuple(background_shape) == per_star:
            sky_mode = 1
        elif tuple(background_shape) == ishape:
            sky_mode = 2
        else:
            raise ValueError(f"background shape {tuple(background_shape)}: a number, one value per "
                             f"star {per_star} or a map {ishape}")
    return dict(batched=batched, B=B, H=ishape[-2], W=ishape[-1], n=n, counts=cnt, hw=int(hw),
                ngauss=int(ngauss), ldeg=int(ldeg), sdeg=int(sdeg), ncomp=ncomp, nterm=nterm,
                shape=shp, sigma_inc=float(sigma_inc), fitrad=float(fitrad), niter=int(niter),
                nsig=float(nsig), min_stars=int(min_stars), origin=(float(org[0]), float(org[1])),
                sky_mode=sky_mode)


class PSFFit:
    """Result of :func:`fit_psf`.  ``coeffs`` [P] (NaN for a singular frame),
    ``psf`` (a :class:`PSF`, or None for a singular frame), per star ``used``
    (bool), ``status`` (``BSGP_PSFFIT_*`` bits), ``rms`` (of the residual per
    fit pixel, in units of the star's flux), ``flux`` (the flux the star was
    divided by) and ``npix``; per frame ``rounds`` (clipping rounds applied),
    ``nused`` and ``frame_status`` (0 or ``BSGP_PSFFIT_SINGULAR``).  For a
    batch ``coeffs`` is [B, P], ``psf`` a list and every per-star attribute a
    list over the frames, each as long as the frame's count; the per-frame
    ones are arrays [B].  With ``device_out=True`` the per-star attributes and
    ``coeffs`` are CUDA tensors ([B, n] views for a batch) and only ``psf``,
    built on first use, waits for the device.  :meth:`refit` solves again from
    the kept moments, without reading a pixel."""

    def __init__(self, cfg, dev, device_out):
        self._cfg, self._dev, self._device_out = cfg, dev, device_out
        self._psf = None
        batched, cnt = cfg["batched"], cfg["counts"]
        names = ("used", "status", "rms", "flux", "npix")
        if device_out:
            coef, frame = dev["coef"], dev["frame"]
            per = {k: dev[k] for k in names}
        else:
            h = _B.to_host({k: dev[k] for k in names + ("coef", "frame")})  # waits
            coef, frame = h["coef"], h["frame"]
            per = {k: [h[k][b, :cnt[b]] for b in range(cfg["B"])] for k in names}
        for k, v in per.items():
            setattr(self, k, v if batched else v[0])
        self.used = [u != 0 for u in self.used] if batched and not device_out else self.used != 0
        self.coeffs = coef if batched else coef[0]
        cols = [frame[:, k] if batched else frame[0, k] for k in range(3)]
        if not device_out and not batched:
            cols = [int(v) for v in cols]
        self.frame_status, self.rounds, self.nused = cols
        if not device_out:
            bad = np.flatnonzero(frame[:, 0] & _B.BSGP_PSFFIT_SINGULAR)
            if len(bad):
                warnings.warn(f"fit_psf: the normal matrix of frame(s) {bad.tolist()} is singular "
                              "(too few usable stars, or stars that do not span the spatial "
                              "terms): no PSF for them", RuntimeWarning, stacklevel=3)

    def _make_psf(self, coef):
        c = self._cfg
        if not np.all(np.isfinite(coef)):
            return None
        return PSF.from_values(c["hw"], c["ngauss"], c["ldeg"], c["sdeg"], *c["shape"],
                               c["sigma_inc"], c["origin"][0], c["origin"][1], coef,
                               fitrad=c["fitrad"])

    @property
    def psf(self):
        if self._psf is None:
            coef = self._dev["coef"].cpu().numpy() if self._device_out else \
                np.atleast_2d(self.coeffs)
            fs = self._dev["frame"].cpu().numpy()[:, 0] if self._device_out else \
                np.atleast_1d(self.frame_status)
            if self._device_out and np.any(fs & _B.BSGP_PSFFIT_SINGULAR):
                warnings.warn("fit_psf: a frame's normal matrix is singular: no PSF for it",
                              RuntimeWarning, stacklevel=2)
            self._psf = [None if s & _B.BSGP_PSFFIT_SINGULAR else self._make_psf(c)
                         for c, s in zip(coef, fs)]
        return self._psf if self._cfg["batched"] else self._psf[0]

    def refit(self, weights=None, niter=0, nsig=2.0, min_stars=None, device_out=None):
        """Solve again from the moments of this fit with other weights or
        another clipping (``bsgp_psf_fit_solve`` alone)."""
        c = dict(self._cfg)
        chk = check_fit_args((c["B"], c["H"], c["W"]) if c["batched"] else (c["H"], c["W"]),
                             (c["B"], c["n"], 2) if c["batched"] else (c["n"], 2), hw=c["hw"],
                             ngauss=c["ngauss"], ldeg=c["ldeg"], sdeg=c["sdeg"], shape=c["shape"],
                             niter=niter, nsig=nsig, min_stars=min_stars,
                             weights_shape=None if weights is None else np.shape(weights))
        c.update(niter=chk["niter"], nsig=chk["nsig"], min_stars=chk["min_stars"])
        dev = dict(self._dev)
        if weights is None:
            dev["weights"] = None
        else:
            w = np.zeros((c["B"], max(1, c["n"])))
            w[:, :c["n"]] = np.asarray(weights, dtype=np.float64).reshape(c["B"], c["n"])
            dev["weights"] = _B.to_dev(w)
        _fit_solve_dev(c, dev)
        return PSFFit(c, dev, self._device_out if device_out is None else device_out)


def _fit_model(c):
    return _B.PsfModel(hw=c["hw"], ngauss=c["ngauss"], ldeg=c["ldeg"], sdeg=c["sdeg"],
                       cos=c["shape"][0], sin=c["shape"][1], ax=c["shape"][2], ay=c["shape"][3],
                       sigma_inc=c["sigma_inc"], x_orig=c["origin"][0], y_orig=c["origin"][1],
                       coeffs=None, ncoef=0)


def _fit_moments_dev(c, dev, sat_level):
    """bsgp_psf_fit_moments on the tensors of ``dev``; adds G, h, vv, npix,
    flux and mstatus.  Asynchronous."""
    torch = _B.torch
    B, n, nc = c["B"], max(1, c["n"]), c["ncomp"]
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    dev.update(G=torch.empty((B, n, nc * (nc + 1) // 2), **f64), h=torch.empty((B, n, nc), **f64),
               vv=torch.empty((B, n), **f64), flux=torch.empty((B, n), **f64),
               npix=torch.empty((B, n), **i32), mstatus=torch.empty((B, n), **i32))
    m = _fit_model(c)
    img = dev["image"]
    _B.check(_B.lib().bsgp_psf_fit_moments(
        _B._ptr(img), _B.BSGP_DTYPE_F32 if img.dtype == torch.float32 else _B.BSGP_DTYPE_F64,
        B, c["H"], c["W"], _B._ptr(dev["xy"]), _B._ptr(dev["counts"]), n, _B.ctypes.byref(m),
        c["fitrad"], _B._ptr(dev["flux_in"]), _B._ptr(dev["sky"]), c["sky_mode"],
        _B._ptr(dev["mask"]), int(sat_level is not None),
        0.0 if sat_level is None else float(sat_level), _B._ptr(dev["G"]), _B._ptr(dev["h"]),
        _B._ptr(dev["vv"]), _B._ptr(dev["npix"]), _B._ptr(dev["flux"]), _B._ptr(dev["mstatus"]),
        _B.current_stream()))


def _fit_solve_dev(c, dev):
    """bsgp_psf_fit_solve on the moments in ``dev``; adds coef, used, status,
    rms and frame.  Asynchronous."""
    torch = _B.torch
    B, n, P = c["B"], max(1, c["n"]), c["ncomp"] * c["nterm"]
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    dev.update(coef=torch.empty((B, P), **f64), used=torch.empty((B, n), **i32),
               status=torch.empty((B, n), **i32), rms=torch.empty((B, n), **f64),
               frame=torch.empty((B, 3), **i32))
    m = _fit_model(c)
    _B.check(_B.lib().bsgp_psf_fit_solve(
        B, n, _B._ptr(dev["counts"]), _B._ptr(dev["xy"]), _B.ctypes.byref(m), _B._ptr(dev["G"]),
        _B._ptr(dev["h"]), _B._ptr(dev["vv"]), _B._ptr(dev["npix"]), _B._ptr(dev["mstatus"]),
        _B._ptr(dev.get("weights")), c["niter"], c["nsig"], c["min_stars"], _B._ptr(dev["coef"]),
        _B._ptr(dev["used"]), _B._ptr(dev["status"]), _B._ptr(dev["rms"]), _B._ptr(dev["frame"]),
        _B.current_stream()))


def _fit_positions(p):
    """Host float64 positions in (x, y): an array, an (x, y) tuple of columns,
    or a catalogue with ``xcentroid`` / ``ycentroid``."""
    if isinstance(p, tuple) and len(p) == 2 and np.ndim(p[0]) == 1:
        return np.stack([np.asarray(p[0], dtype=np.float64), np.asarray(p[1], dtype=np.float64)],
                        axis=1)
    if isinstance(p, (np.ndarray, list)):
        return np.asarray(p, dtype=np.float64)
    if _B.torch is not None and _B.torch.is_tensor(p):
        return p.detach().cpu().numpy().astype(np.float64)
    import segmentation  # the catalogue's columns, as validate_sources reads them
    return segmentation._positions_of(p)


def _fit_image_dev(a, keep_f32=True):
    torch = _B.torch
    if torch.is_tensor(a):
        t = a.to("cuda")
        if t.dtype != torch.float64 and not (keep_f32 and t.dtype == torch.float32):
            t = t.to(torch.float64)
        return t.contiguous()
    a = np.asarray(a)
    if a.dtype != np.float64 and not (keep_f32 and a.dtype == np.float32):
        a = a.astype(np.float64)
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.copy() if not a.flags.writeable else a).to("cuda")


def fit_psf(image, positions, hw=15, ngauss=2, ldeg=2, sdeg=1, fwhm=None, shape=None,
            sigma_inc=SIGMA_INC, fitrad=None, flux=None, background=0.0, mask=None, sat_level=None,
            weights=None, niter=0, nsig=2.0, min_stars=None, origin=None, counts=None,
            device_out=False):
    """Fit the DIAPL PSF model to the stars of a frame, on the device: what the
    reference leaves to DIAPL's ``getpsf`` (psf/psf_estimation.bash; the
    defaults are getpsf.par's: hw = PSFHW = 15, two Gaussians, local degree 2,
    spatial degree 1, sigma_inc 0.548).  DESIGN §3.14, P1 to P8.

    ``image``: [H, W] float32 or float64 with ``positions`` [n, 2] in 0-based
    (x, y), x the column (an array, a :class:`segmentation.SourceCatalog`, or an
    (x, y) tuple), or a batch [B, H, W] with positions [B, n, 2] and
    ``counts`` [B].  The shape parameters are inputs: ``shape=(cos, sin, ax,
    ay)`` or a circular ``fwhm``.  With them fixed the model is linear in its
    coefficients: per star the pixels of the (2 hw + 1)^2 box within ``fitrad``
    (default hw) of the position, minus ``background`` (a number, one per star
    or a map; default 0: a background-subtracted frame) and divided by the
    star's ``flux`` (default: their sum), give the moments of one weighted
    least-squares problem per frame, solved by a scaled Cholesky
    factorisation.  Pixels that are not finite, masked (``mask`` nonzero) or
    at or above ``sat_level`` are left out.  ``weights``: one per star.
    ``niter`` clipping rounds (NITER; default 0) drop the stars whose residual
    rms is above median + ``nsig`` * 1.4826 * MAD and repeat the fit, while at
    least ``max(nterm, min_stars)`` remain.  ``origin`` of the spatial
    expansion: (W / 2, H / 2) by default.

    Not done: the shape parameters are not fitted, the stars are not
    recentred or cleaned of neighbours, and pixels carry no noise weights.
    Choosing the stars is ``starfind.select_psf_stars``, whose
    ``StarList.psf_inputs(sel)`` are this function's ``positions``, ``flux``
    and ``background``.  Returns a :class:`PSFFit`; a singular frame warns and has no
    ``psf``."""
    torch = _B.torch
    ishape = tuple(image.shape)
    pos = _fit_positions(positions)
    bg_shape = () if np.ndim(background) == 0 else tuple(np.shape(background))
    c = check_fit_args(ishape, pos.shape, hw, ngauss, ldeg, sdeg, fwhm, shape, sigma_inc, fitrad,
                       niter, nsig, min_stars, origin, counts,
                       None if mask is None else tuple(mask.shape),
                       None if flux is None else np.shape(flux),
                       None if weights is None else np.shape(weights), bg_shape, sat_level)
    _B.require_gpu()
    B, n, H, W = c["B"], c["n"], c["H"], c["W"]
    cap = max(1, n)

    def per_star(v):
        a = np.zeros((B, cap))
        a[:, :n] = np.asarray(v, dtype=np.float64).reshape(B, n)
        return _B.to_dev(a)

    dev = dict(image=_fit_image_dev(image).reshape(B, H, W),
               counts=torch.from_numpy(c["counts"].copy()).to("cuda"), mask=None, sky=None,
               flux_in=None if flux is None else per_star(flux),
               weights=None if weights is None else per_star(weights))
    xy = np.zeros((B, cap, 2))
    xy[:, :n] = pos.reshape(B, n, 2)
    dev["xy"] = _B.to_dev(xy)
    if mask is not None:
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask) != 0)
        dev["mask"] = (m != 0).to(torch.uint8).to("cuda").contiguous().reshape(B, H, W)
    if c["sky_mode"] == 0 and float(background) != 0.0:
        c["sky_mode"] = 1
        dev["sky"] = per_star(np.full((B, n), float(background)))
    elif c["sky_mode"] == 1:
        dev["sky"] = per_star(background)
    elif c["sky_mode"] == 2:
        dev["sky"] = _fit_image_dev(background, keep_f32=False).reshape(B, H, W)
    _fit_moments_dev(c, dev, sat_level)
    _fit_solve_dev(c, dev)
    return PSFFit(c, dev, device_out)
