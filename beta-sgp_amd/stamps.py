"""Star-stamp metrics on the device: radial profiles, Gaussian fits and the
Wasserstein distance of the fitted profiles.

The reference computes them per star with numpy, astropy and scipy
(restoration/application_sgp_star_stamps.py:117-142, through
``utils.radial_profile``, ``utils.fit_radprof`` and
``utils.wasserstein_distance_norm``, restoration/utils.py:81-92, 180-202,
276-291).  The functions here keep those names and call ``bsgp_radial_profile``,
``bsgp_fit_gauss1d`` and ``bsgp_wasserstein1`` (include/bsgp.h; semantics in
DESIGN §3.9) for one stamp or a batch; :func:`stamp_metrics` chains them for a
batch without a host synchronisation in between.

The application's loop around them (:56-148) is here as well:
:func:`cutout_stamps` (``Cutout2D`` at float positions, ``bsgp_extract_stamps``),
:func:`select_single_source` (the ``len(scat) == 1`` selection) and the driver
:func:`sgp_star_stamps`, which chains the cutouts, the selection, ONE batched
solve of every (star, candidate), the restored catalogue, the choice among the
candidates on the device (``bsgp_stamp_select``) and the metrics (DESIGN
§3.11).

``center`` is ``(c0, c1)`` with ``c0`` measured along the rows (axis 0), as
the reference's ``np.indices`` order has it; the reference passes
``(xcentroid, ycentroid)`` there, and that quirk is kept: pass what the
reference passes to get what it gets.
"""
import numpy as np

import _bsgp as _B

MAX_PIXELS = 16384  # H * W of one stamp
MAX_BINS = 256      # radial bins, profile length, sample length
CUT_MAX_PIXELS = 1 << 24  # sh * sw of one cutout
BOX_LIMIT = 1 << 30       # |imin| of a cutout's box (include/bsgp.h)
# columns of a bsgp_stamp_select result row
ROW_COLUMNS = ("orig_flux", "restored_flux", "flux_fractional_difference", "fwhm_ratio",
               "ellipticity_ratio", "orig_xcentroid", "orig_ycentroid", "orig_fwhm",
               "restored_xcentroid", "restored_ycentroid", "restored_fwhm")
assert len(ROW_COLUMNS) == _B.BSGP_STAMP_ROW_COLS


def _shape_of(a):
    torch = _B.torch
    return tuple(a.shape) if torch is not None and torch.is_tensor(a) else np.shape(a)


def _host(a):
    torch = _B.torch
    return a.detach().cpu().numpy() if torch is not None and torch.is_tensor(a) else np.asarray(a)


def profile_reach(shape, centers):
    """The distance of the farthest pixel (a corner) of an [H, W] image from
    each centre, as the profile computes it (host only): its truncation + 1 is
    the number of bins."""
    H, W = shape
    c = np.asarray(centers, np.float64).reshape(-1, 2)
    rows = np.array([0.0, 0.0, H - 1.0, H - 1.0])
    cols = np.array([0.0, W - 1.0, 0.0, W - 1.0])
    with np.errstate(over="ignore"):
        return np.sqrt((rows[None] - c[:, :1]) ** 2 + (cols[None] - c[:, 1:]) ** 2).max(axis=1)


def check_profile_args(shape, centers):
    """The argument checks of radial_profile (host only): returns
    (batched, centers [B, 2] float64, rcap)."""
    if len(shape) not in (2, 3) or 0 in shape:
        raise ValueError(f"data must be [H, W] or [B, H, W], got shape {tuple(shape)}")
    batched = len(shape) == 3
    B = shape[0] if batched else 1
    H, W = shape[-2:]
    if H * W > MAX_PIXELS:
        raise ValueError(f"a stamp holds at most {MAX_PIXELS} pixels, got {H} x {W}")
    c = np.asarray(centers, np.float64)
    if c.shape == (2,):
        c = np.broadcast_to(c, (B, 2))
    if c.shape != (B, 2):
        raise ValueError(f"center must be a pair or [B, 2] for B = {B}, got shape {c.shape}")
    if not np.all(np.isfinite(c)):
        raise ValueError("center must be finite")
    reach = float(profile_reach((H, W), c).max())
    rcap = int(reach) + 1 if reach < MAX_BINS else MAX_BINS + 1
    if rcap > MAX_BINS:
        raise ValueError(f"a radial profile holds at most {MAX_BINS} bins; the centre(s) and the "
                         f"shape {H} x {W} give more")
    return batched, np.ascontiguousarray(c), rcap


def check_fwhm(fwhm, B):
    """fwhm as a float64 [B] array: positive and finite (host only)."""
    f = np.asarray(fwhm, np.float64)
    if f.ndim == 0:
        f = np.broadcast_to(f, (B,))
    if f.shape != (B,):
        raise ValueError(f"fwhm must be a number or [B] for B = {B}, got shape {f.shape}")
    if not np.all(np.isfinite(f) & (f > 0)):
        raise ValueError("fwhm must be positive and finite")
    return np.ascontiguousarray(f)


def check_samples(shape, lengths, name):
    """A sample array [n] or [B, R] and its optional lengths (host only):
    returns (batched, B, R)."""
    if len(shape) not in (1, 2) or 0 in shape:
        raise ValueError(f"{name} must be [n] or [B, R], got shape {tuple(shape)}")
    batched = len(shape) == 2
    B, R = (shape if batched else (1, shape[0]))
    if R > MAX_BINS:
        raise ValueError(f"{name} holds at most {MAX_BINS} values per row, got {R}")
    if lengths is not None and _shape_of(lengths) != (B,) and not (not batched and _shape_of(lengths) == ()):
        raise ValueError(f"the lengths of {name} must be [B] for B = {B}, got shape {_shape_of(lengths)}")
    return batched, B, R


def _dev_f64(a, shape=None):
    torch = _B.torch
    if torch.is_tensor(a):
        t = a.to(device="cuda", dtype=torch.float64)
    else:
        t = torch.from_numpy(np.require(a, np.float64, ["C", "W"])).to("cuda")
    return (t if shape is None else t.reshape(shape)).contiguous()


def _dev_i32(a, B):
    torch = _B.torch
    if torch.is_tensor(a):
        t = a.to(device="cuda", dtype=torch.int32)
    else:
        t = torch.from_numpy(np.require(a, np.int32, ["C", "W"])).to("cuda")
    return t.reshape(B).contiguous()


def _images(data):
    """float32 / float64 CUDA tensor [B, H, W]."""
    torch = _B.torch
    if torch.is_tensor(data):
        d = data if data.dtype in (torch.float32, torch.float64) else data.to(torch.float64)
        d = d.to("cuda").contiguous()
    else:
        d = np.asarray(data)
        if not (d.dtype.kind == "f" and d.dtype.itemsize in (4, 8)):
            d = d.astype(np.float64)
        d = torch.from_numpy(np.require(d.astype(d.dtype.newbyteorder("="), copy=False), None, ["C", "W"])).to("cuda")
    return d if d.dim() == 3 else d[None]


# ---------------------------------------------------------------- device calls
def _profile_dev(d, centers, rcap):
    torch = _B.torch
    B, H, W = d.shape
    prof = torch.empty((B, rcap), dtype=torch.float64, device="cuda")
    length = torch.empty((B,), dtype=torch.int32, device="cuda")
    c = _dev_f64(centers, (B, 2))
    dtype = _B.BSGP_DTYPE_F32 if d.dtype == torch.float32 else _B.BSGP_DTYPE_F64
    _B.check(_B.lib().bsgp_radial_profile(_B._ptr(d), dtype, B, H, W, _B._ptr(c), rcap,
                                          _B._ptr(prof), _B._ptr(length), _B.current_stream()))
    return prof, length


def _fit_dev(prof, length, fwhm):
    torch = _B.torch
    B, rcap = prof.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    fitted, params, perr = torch.empty((B, rcap), **f64), torch.empty((B, 3), **f64), \
        torch.empty((B, 3), **f64)
    info = torch.empty((B, 2), dtype=torch.int32, device="cuda")
    _B.check(_B.lib().bsgp_fit_gauss1d(_B._ptr(prof), _B._ptr(length), B, rcap, _B._ptr(fwhm),
                                       _B._ptr(fitted), _B._ptr(params), _B._ptr(perr),
                                       _B._ptr(info), _B.current_stream()))
    return fitted, params, perr, info


def _w1_dev(u, ulen, v, vlen):
    torch = _B.torch
    B, rcap = u.shape
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    _B.check(_B.lib().bsgp_wasserstein1(_B._ptr(u), _B._ptr(ulen), _B._ptr(v), _B._ptr(vlen), B,
                                        rcap, _B._ptr(out), _B.current_stream()))
    return out


def _pad_to(t, R):
    """[B, r] -> [B, R] (r <= R), the new columns NaN."""
    torch = _B.torch
    if t.shape[1] == R:
        return t
    out = torch.full((t.shape[0], R), float("nan"), dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


# ------------------------------------------------------------------- interface
def radial_profile(data, center, device_out=False):
    """``utils.radial_profile(data, center)``: the mean of the pixels at each
    truncated distance from ``center`` (module docstring: ``center[0]`` runs
    along the rows).  One [H, W] image gives a Python list, as the reference's
    ``.tolist()`` does (a CUDA tensor with ``device_out=True``); a batch
    [B, H, W] with ``center`` a pair or [B, 2] gives ``(profiles [B, R],
    lengths [B])``, a profile being NaN from its length on.  An empty bin
    inside a profile is NaN (0 / 0), as in numpy.  float32 or float64 input,
    widened first; H * W <= 16384, at most 256 bins."""
    batched, c, rcap = check_profile_args(_shape_of(data), _host(center))
    _B.require_gpu()
    prof, length = _profile_dev(_images(data), c, rcap)
    if batched:
        return (prof, length) if device_out else (prof.cpu().numpy(), length.cpu().numpy())
    # (one image: rcap is its length)
    return prof[0] if device_out else prof[0].cpu().numpy().tolist()


def _fwhm_of(fwhm_or_table):
    """A number or array as it is; of anything indexable by 'fwhm' (a
    SourceCatalog, an astropy table) element 0 of that column, as the
    reference's ``table['fwhm'].value[0]``."""
    torch = _B.torch
    if isinstance(fwhm_or_table, (int, float, np.ndarray, list, tuple, np.generic)) or (
            torch is not None and torch.is_tensor(fwhm_or_table)):
        return _host(fwhm_or_table)
    col = fwhm_or_table["fwhm"]
    col = getattr(col, "value", col)
    return np.asarray(np.ravel(_host(col))[0])


def fit_radprof(radprof, fwhm_or_table, lengths=None, device_out=False, full=False):
    """``utils.fit_radprof(radprof, table)``: a ``Gaussian1D`` fitted to the
    profile over x = 0 .. len-1 from amplitude 0.8 max, mean 0 and stddev
    fwhm / (2 sqrt(2 ln 2)), by MINPACK's lmder with the settings astropy's
    ``LevMarLSQFitter`` gives it.  Returns ``(fitted,
    param_errs)``; with ``full=True`` also ``params`` (amplitude, mean, stddev),
    ``ier`` and ``nfev``.  ``radprof``: [n] (a list, as radial_profile returns
    it) or [B, R] with ``lengths`` [B] (default: R).  ``fwhm_or_table``: a
    number, [B], or anything indexable by ``'fwhm'``, of which element 0 is
    used.  ``param_errs`` is NaN where the reference falls back to NaN (no
    covariance) or the profile has 3 values; a profile shorter than 3 or with a
    non-finite value gives ier 0 and NaNs."""
    batched, B, R = check_samples(_shape_of(radprof), lengths, "radprof")
    fw = check_fwhm(_fwhm_of(fwhm_or_table), B)
    _B.require_gpu()
    torch = _B.torch
    prof = _dev_f64(radprof, (B, R))
    length = (torch.full((B,), R, dtype=torch.int32, device="cuda") if lengths is None
              else _dev_i32(lengths, B))
    fitted, params, perr, info = _fit_dev(prof, length, _dev_f64(fw, (B,)))
    res = (fitted, perr, params, info[:, 0], info[:, 1]) if full else (fitted, perr)
    if not batched:
        res = tuple(t[0] for t in res)
    return res if device_out else tuple(t.cpu().numpy() for t in res)


def wasserstein_distance_norm(p, q, p_len=None, q_len=None, device_out=False):
    """``utils.wasserstein_distance_norm(p, q)``, that is
    ``scipy.stats.wasserstein_distance(p, q)``: [n] and [m] give a float, [B, R]
    and [B, S] with ``p_len`` / ``q_len`` [B] (default: R, S) give [B].  NaN for
    a non-finite value inside a length.  At most 256 values per sample."""
    pb, B, R = check_samples(_shape_of(p), p_len, "p")
    qb, Bq, S = check_samples(_shape_of(q), q_len, "q")
    if pb != qb or B != Bq:
        raise ValueError(f"p and q must both be samples or batches of one size, got shapes "
                         f"{_shape_of(p)} and {_shape_of(q)}")
    _B.require_gpu()
    torch = _B.torch
    cap = max(R, S)
    u, v = _pad_to(_dev_f64(p, (B, R)), cap), _pad_to(_dev_f64(q, (B, S)), cap)
    ulen = (torch.full((B,), R, dtype=torch.int32, device="cuda") if p_len is None
            else _dev_i32(p_len, B))
    vlen = (torch.full((B,), S, dtype=torch.int32, device="cuda") if q_len is None
            else _dev_i32(q_len, B))
    out = _w1_dev(u.contiguous(), ulen, v.contiguous(), vlen)
    if not pb:
        return out[0] if device_out else float(out[0].cpu())
    return out if device_out else out.cpu().numpy()


def stamp_metrics(orig_sub, restored_sub, orig_center, restored_center, orig_fwhm, restored_fwhm,
                  device_out=False):
    """Lines 118-142 of the star-stamp application for a batch: the radial
    profiles of the background-subtracted observed and restored stamps
    ([B, H, W] and [B, H2, W2]) about their centres ([B, 2] or a pair), the
    Gaussian fit of each from its FWHM ([B] or a number) and the Wasserstein
    distance of the two fitted profiles.  Two profile calls, two fits and one
    distance on the current stream, the lengths staying on the device and no
    host synchronisation between those launches.  Centres and FWHMs are read on
    the host before the first one (it sizes the profiles from the centres):
    pass them as host arrays; device tensors are copied back first, which
    waits for the stream.  Returns a dict: ``orig_radprof``,
    ``restored_radprof`` [B, R] (NaN from ``orig_len`` / ``restored_len`` on;
    R is the larger of the two widths), ``fitted_orig``, ``fitted_restored``,
    ``ier``, ``nfev`` [B, 2] (observed, restored) and ``wd`` [B]; numpy arrays,
    or CUDA tensors with ``device_out=True``."""
    so, sr = _shape_of(orig_sub), _shape_of(restored_sub)
    if len(so) != 3 or len(sr) != 3 or so[0] != sr[0]:
        raise ValueError(f"orig_sub and restored_sub must be [B, H, W] batches of one size, got "
                         f"shapes {so} and {sr}")
    B = so[0]
    _, co, ro = check_profile_args(so, _host(orig_center))
    _, cr, rr = check_profile_args(sr, _host(restored_center))
    fo, fr = check_fwhm(_host(orig_fwhm), B), check_fwhm(_host(restored_fwhm), B)
    _B.require_gpu()
    torch = _B.torch
    rcap = max(ro, rr)
    po, lo = _profile_dev(_images(orig_sub), co, rcap)
    pr, lr = _profile_dev(_images(restored_sub), cr, rcap)
    fito, _, _, io = _fit_dev(po, lo, _dev_f64(fo, (B,)))
    fitr, _, _, ir = _fit_dev(pr, lr, _dev_f64(fr, (B,)))
    wd = _w1_dev(fito, lo, fitr, lr)
    out = {"orig_radprof": po, "restored_radprof": pr, "orig_len": lo, "restored_len": lr,
           "fitted_orig": fito, "fitted_restored": fitr,
           "ier": torch.stack((io[:, 0], ir[:, 0]), 1), "nfev": torch.stack((io[:, 1], ir[:, 1]), 1),
           "wd": wd}
    return out if device_out else _B.to_host(out)


# ------------------------------------------------- cutouts, selection, driver
def _stamp_size(size):
    ok = (int, np.integer)
    if isinstance(size, ok) and not isinstance(size, (bool, np.bool_)):
        size = (size, size)
    if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(
            isinstance(v, ok) and not isinstance(v, (bool, np.bool_)) for v in size)):
        raise ValueError(f"size must be an int or a pair (ny, nx) of ints, got {size!r}")
    sh, sw = int(size[0]), int(size[1])
    if sh < 1 or sw < 1:
        raise ValueError(f"size must be positive, got {size!r}")
    if sh * sw > CUT_MAX_PIXELS:
        raise ValueError(f"a cutout holds at most {CUT_MAX_PIXELS} pixels, got {sh} x {sw}")
    return sh, sw


def check_cutout_args(shape, positions, size):
    """The argument checks of cutout_stamps (host only): returns ((H, W),
    positions [n, 2] float64, (sh, sw)).  A non-finite coordinate is no error:
    it gets a status bit."""
    if len(shape) != 2 or 0 in shape:
        raise ValueError(f"image must be [H, W], got shape {tuple(shape)}")
    try:
        p = np.asarray(positions, np.float64)
    except (TypeError, ValueError):
        raise ValueError("positions must be numbers, [n, 2] in (x, y)") from None
    if p.shape == (0,):  # an empty list
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"positions must be [n, 2] in (x, y), got shape {p.shape}")
    return (int(shape[0]), int(shape[1])), np.ascontiguousarray(p), _stamp_size(size)


def cutout_stamps(image, positions, size=31, device_out=False):
    """``Cutout2D(image, (x, y), size)`` (mode 'trim') at every row of
    ``positions`` [n, 2] in ``(x, y)``, x the column
    (application_sgp_star_stamps.py:58): ``bsgp_extract_stamps``, one launch.
    ``image``: 2-D float32 or float64 (kept, so that a float32 frame keeps the
    reference's float32 arithmetic) or integer (widened to float64), numpy or
    CUDA tensor.  ``size``: an int or ``(ny, nx)``.  The box is astropy 4.3.1's:
    per axis it starts at ``ceil(pos - size / 2)``.  Returns ``(stamps
    [n, ny, nx], boxes [n, 4], status [n])``: the untrimmed ``x0, y0, x1, y1``
    and 0 or one of ``BSGP_STAMP_PARTIAL`` (the box leaves the image; the pixels
    outside are 0 -- the reference drops such a stamp), ``BSGP_STAMP_NO_OVERLAP``
    (astropy raises; all 0) and ``BSGP_STAMP_BAD_POSITION`` (a non-finite
    coordinate; all 0).  numpy arrays, or CUDA tensors with ``device_out=True``."""
    (H, W), pos, (sh, sw) = check_cutout_args(_shape_of(image), _host(positions), size)
    _B.require_gpu()
    torch = _B.torch
    img = _images(image)[0]
    n = len(pos)
    out = torch.empty((n, sh, sw), dtype=img.dtype, device="cuda")
    box = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    if n:
        xy = _dev_f64(pos, (n, 2))
        dtype = _B.BSGP_DTYPE_F32 if img.dtype == torch.float32 else _B.BSGP_DTYPE_F64
        _B.check(_B.lib().bsgp_extract_stamps(_B._ptr(img), dtype, H, W, _B._ptr(xy), n, sh, sw,
                                              _B._ptr(out), _B._ptr(box), _B._ptr(st),
                                              _B.current_stream()))
    if device_out:
        return out, box, st
    res = _B.to_host({"s": out, "b": box, "t": st})
    return res["s"], res["b"], res["t"]


def select_single_source(stamps, box_size=(5, 5), n_pixels=5, localbkg_width=5, deblend=True):
    """The application's selection (application_sgp_star_stamps.py:63-66): one
    batched ``source_info`` over ``stamps`` [B, H, W] and the mask of the
    stamps whose catalogue holds exactly one source.  The defaults are
    ``utils.source_info``'s own (restoration/utils.py:219, 235, 245: 5 x 5
    boxes, 5 pixels, ``SourceFinder(deblend=True)``, ``localbkg_width=5``).  The
    application's call ``source_info(cutout.data, localbkg_width=5)`` is stale
    against that signature (it takes no such keyword); what it means is
    what the function does anyway.  Returns ``(catalog, background, mask)``, the
    first two as ``segmentation.source_info(..., device_out=True)`` returns
    them, ``mask = catalog.nlabels == 1`` on the host."""
    import segmentation
    if len(_shape_of(stamps)) != 3:
        raise ValueError(f"stamps must be a batch [B, H, W], got shape {_shape_of(stamps)}")
    cat, bkg = segmentation.source_info(stamps, box_size, n_pixels, device_out=True,
                                        deblend=deblend, localbkg_width=localbkg_width)
    return cat, bkg, np.asarray(cat.nlabels) == 1


def _select_dev(nlabels, res_cols, obs_cols, iters, n, K):
    """bsgp_stamp_select on device tensors: res_cols [n * K, cap, 8], obs_cols
    [n, cap, 8], nlabels and iters int32 [n * K]."""
    torch = _B.torch
    scores = torch.empty((n, K), dtype=torch.float64, device="cuda")
    rows = torch.empty((n, _B.BSGP_STAMP_ROW_COLS), dtype=torch.float64, device="cuda")
    best, nit, st = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(3))
    _B.check(_B.lib().bsgp_stamp_select(
        _B._ptr(nlabels), _B._ptr(res_cols), res_cols.shape[1] * 8, _B._ptr(obs_cols),
        obs_cols.shape[1] * 8, _B._ptr(iters), n, K, _B._ptr(scores), _B._ptr(best), _B._ptr(rows),
        _B._ptr(nit), _B._ptr(st), _B.current_stream()))
    return scores, best, rows, nit, st


def stamp_select(res_nlabels, res_cols, obs_cols, iters, K, device_out=False):
    """The choice among the K restorations of each star and its result row
    (application_sgp_star_stamps.py:92-98, 125-139; ``bsgp_stamp_select``).
    Image ``s * K + k`` is candidate k of star s.  ``res_nlabels`` [n * K] and
    ``res_cols`` [n * K, cap, 8]: the detections and the ``f64_cols`` of the
    restored catalogue; ``obs_cols`` [n, cap, 8]: those of the observed one (row
    0, label 1, is read); ``iters`` [n * K].  Returns ``(scores [n, K], best [n],
    rows [n, 11], num_iters [n], status [n])``: ``best`` is
    ``sgp.argmin_strict`` of the star's scores (-1 for its None), ``rows`` has
    the columns ``ROW_COLUMNS``."""
    torch = _B.torch
    n = int(_shape_of(obs_cols)[0])
    if K < 1 or _shape_of(res_cols)[:1] != (n * K,) or _shape_of(res_cols)[2:] != (8,) \
            or _shape_of(obs_cols)[2:] != (8,) or len(_shape_of(res_cols)) != 3:
        raise ValueError(f"res_cols must be [n * K, cap, 8] and obs_cols [n, cap, 8] for K = {K}, "
                         f"got shapes {_shape_of(res_cols)} and {_shape_of(obs_cols)}")
    if _shape_of(res_nlabels) != (n * K,) or _shape_of(iters) != (n * K,):
        raise ValueError(f"res_nlabels and iters must be [n * K] = [{n * K}]")
    _B.require_gpu()
    out = _select_dev(_dev_i32(res_nlabels, n * K), _dev_f64(res_cols), _dev_f64(obs_cols),
                      _dev_i32(iters, n * K), n, K)
    if device_out:
        return out
    res = _B.to_host(dict(enumerate(out)))
    return tuple(res[i] for i in range(5))


RESULT_KEYS = ("ORIG_FLUX", "RESTORED_FLUX", "FLUX_FRACTIONAL_DIFFERENCE", "FWHM_RATIO",
               "ELLIPTICITY_RATIO", "WD_RADIAL_PROFILE_DISTANCE", "NUM_ITERS", "EXEC_TIME")


def star_stamp_kwargs(use_betadiv=True):
    """The keywords of the application's solver calls
    (application_sgp_star_stamps.py:82-89 and 107-112): DEFAULT_PARAMS unpacked
    (:23), flux projection, start from the data, stop rule 3, saturation at
    65000, scaled data, the circular A; for sgp_betaDiv also the adaptive beta
    with its scheduled learning rate."""
    import sgp
    max_projs, gamma, beta, alpha_min, alpha_max, alpha, M_alpha, tau, M = sgp.DEFAULT_PARAMS
    kw = dict(gamma=gamma, beta=beta, alpha_min=alpha_min, alpha_max=alpha_max, alpha=alpha,
              M_alpha=M_alpha, tau=tau, M=M, max_projs=max_projs, proj_type=1, init_recon=2,
              stop_criterion=3, ccd_sat_level=65000, scale_data=True,
              use_original_SGP_Afunction=True)
    if use_betadiv:
        kw.update(lr=1e-3, lr_exp_param=0.1, schedule_lr=True, adapt_beta=True)
    return kw


def _empty_result(status, K, shape, device_out):
    torch = _B.torch

    def arr(shp, dt):
        if device_out:
            return torch.empty(shp, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
        return np.empty(shp, dt)

    res = {k: arr((0,), np.float64) for k in RESULT_KEYS}
    res["NUM_ITERS"] = arr((0,), np.int32)
    res.update(kept=np.empty((0,), np.int64), status=status, best=arr((0,), np.int32),
               best_beta=np.empty((0,), np.float64), scores=arr((0, K), np.float64),
               beta_final=arr((0,), np.float64), x=arr((0,) + tuple(shape), np.float64),
               solver_status=arr((0, K), np.int64), metrics=None)
    return res


def sgp_star_stamps(image, positions, psf, size=31, use_betadiv=True, betas=None, MAXIT=500,
                    device_out=False, **sgp_kwargs):
    """The star-stamp application's loop (application_sgp_star_stamps.py:56-148)
    for one frame and a list of star coordinates ``positions`` [n, 2] in
    ``(x, y)``, with every star's work batched:

    1. :func:`cutout_stamps`; a stamp with a non-zero status is dropped (:60-61).
    2. :func:`select_single_source`; kept are the stamps with exactly one source
       (:65-66) whose ``segment_flux[0]`` is positive (the reference raises on
       another: no positive entry in flux / (flux + bkg) * AT(gn); here it is the
       status bit ``BSGP_STAMP_BAD_FLUX``).
    3. ONE batched solve of (kept stamp x candidate) with ``bkg =
       background_median`` and ``flux = segment_flux[0]`` of the stamp and
       :func:`star_stamp_kwargs`; ``sgp_kwargs`` override those and pass anything
       else ``sgp_betaDiv_batch`` / ``sgp_batch`` take.  The candidates are
       ``betas`` (default ``sgp.app_beta_candidates()``, :69-75);
       ``use_betadiv=False`` is the ``sgp(...)`` branch (:107-112) with one
       candidate.
    4. One batched ``source_info`` of all restored candidates (:90, 114).
    5. ``bsgp_stamp_select``: the scores, the winner (:95-97) and the result row
       of every star on the device; no host round trip decides it.
    6. :func:`stamp_metrics` on the winners' background-subtracted stamps (the
       catalogues' ``data``, gathered by ``best`` on the device).

    The application's final solve (:98-105) repeats the best candidate's run
    exactly, so it is not run again (as in ``sgp.sgp_betaDiv_multistart``).
    The host reads the cutout status and the catalogues (``source_info`` returns
    its columns on the host) before the solve, to size the batch; after the solve
    only ``stamp_metrics`` reads the winners' centres and widths back, to size
    its profiles.

    Returns a dict.  One entry per kept star, in input order: ``ORIG_FLUX``,
    ``RESTORED_FLUX``, ``FLUX_FRACTIONAL_DIFFERENCE``, ``FWHM_RATIO``,
    ``ELLIPTICITY_RATIO``, ``WD_RADIAL_PROFILE_DISTANCE``, ``NUM_ITERS`` (the
    arrays the reference saves), ``best`` (-1: none), ``best_beta``, ``scores``
    [n_kept, K], ``beta_final`` (of the winner; NaN for ``use_betadiv=False``),
    ``x`` (the winners' restored stamps), ``solver_status`` [n_kept, K] (the
    solver's status bits, ``_bsgp.check_status``) and ``metrics`` (the
    :func:`stamp_metrics` dict).  ``EXEC_TIME`` is NOT per star: it is the time
    of the one batched solve (device events around it) divided evenly over the
    kept stars.  ``kept``: their indices into ``positions``.  ``status`` [n]: 0
    for a kept star with a result, else the cutout's bit or one of
    ``BSGP_STAMP_NO_SOURCE``, ``_MULTI_SOURCE``, ``_BAD_FLUX`` (dropped),
    ``_NO_CANDIDATE`` (no candidate's restoration has a detection) and
    ``_RESTORED_NO_SOURCE`` (``use_betadiv=False``: the restoration has none): a
    star with one of the last two keeps its row, with NaN for the restored flux,
    the ratios and the distance and -1 iterations.  One star never makes the
    driver raise; no position, or none that survives, returns empty arrays (and
    ``metrics`` None) without a solve.  numpy arrays, or CUDA tensors with
    ``device_out=True`` (``kept``, ``status`` and ``best_beta`` stay numpy)."""
    import sgp
    torch = _B.torch
    (H, W), pos, (sh, sw) = check_cutout_args(_shape_of(image), _host(positions), size)
    betas = [float(b) for b in (sgp.app_beta_candidates() if betas is None else betas)] \
        if use_betadiv else [float("nan")]
    K = len(betas)
    if K < 1:
        raise ValueError("betas must hold at least one candidate")
    _B.require_gpu()
    n = len(pos)
    if n == 0:
        return _empty_result(np.zeros(0, np.int32), K, (sh, sw), device_out)
    stamps, _, st = cutout_stamps(image, pos, (sh, sw), device_out=True)
    status = st.cpu().numpy().astype(np.int32)
    full = np.flatnonzero(status == 0)
    if full.size == 0:
        return _empty_result(status, K, (sh, sw), device_out)
    cat_o, bkg_o, single = select_single_source(stamps[torch.from_numpy(full).to("cuda")])
    nlab = np.asarray(cat_o.nlabels)
    flux = np.array([f[0] if len(f) else np.nan for f in cat_o.segment_flux], np.float64)
    status[full[nlab == 0]] |= _B.BSGP_STAMP_NO_SOURCE
    status[full[nlab > 1]] |= _B.BSGP_STAMP_MULTI_SOURCE
    keep = single & (flux > 0)
    status[full[single & ~keep]] |= _B.BSGP_STAMP_BAD_FLUX
    kept = full[keep]
    nk = int(kept.size)
    if nk == 0:
        return _empty_result(status, K, (sh, sw), device_out)
    kk = torch.from_numpy(np.flatnonzero(keep)).to("cuda")
    gns = stamps[torch.from_numpy(kept).to("cuda")].repeat_interleave(K, dim=0)
    kw = star_stamp_kwargs(use_betadiv)
    kw.update(sgp_kwargs)
    kw.update(MAXIT=MAXIT, device_out=True,
              flux=np.repeat(flux[keep], K))
    bkgs = np.repeat(np.asarray(bkg_o.background_median, np.float64)[keep], K)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    if use_betadiv:
        out = sgp.sgp_betaDiv_batch(gns, psf, bkgs, betaParams=np.tile(betas, nk), **kw)
    else:
        out = sgp.sgp_batch(gns, psf, bkgs, **kw)
    t1.record()
    # a restoration with a non-finite pixel (source_info refuses those) counts
    # as one without a detection: it is catalogued as an empty image
    xr = out["x"]
    xr = torch.where(torch.isfinite(xr).reshape(nk * K, -1).all(dim=1)[:, None, None], xr,
                     torch.zeros_like(xr))
    cat_r, _, _ = select_single_source(xr)
    nlab_r = torch.from_numpy(np.ascontiguousarray(cat_r.nlabels, np.int32)).to("cuda")
    scores, best, rows, nit, sel = _select_dev(nlab_r, cat_r.f64_cols,
                                               cat_o.f64_cols[kk].contiguous(), out["iters"], nk, K)
    # the winner's image index (candidate 0 stands in where there is none: its
    # results are overwritten with NaN below)
    win = torch.arange(nk, device="cuda") * K + best.clamp(min=0).to(torch.int64)
    none = sel != 0
    rows_h = rows.cpu().numpy()  # the centres and widths size the profiles
    co, fo, cr, fr = rows_h[:, 5:7], rows_h[:, 7], rows_h[:, 8:10], rows_h[:, 10]
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(rows_h[:, 5:]).all(axis=1) & (fo > 0) & (fr > 0))
        bad |= ~(profile_reach((sh, sw), np.where(bad[:, None], 0.0, co)) < MAX_BINS)
        bad |= ~(profile_reach((sh, sw), np.where(bad[:, None], 0.0, cr)) < MAX_BINS)
    # a star without a winner, or with a centre or width no profile can be made
    # from, is measured about (0, 0) with width 1 and its distance set to NaN
    met = stamp_metrics(cat_o.data[kk], cat_r.data[win], np.where(bad[:, None], 0.0, co),
                        np.where(bad[:, None], 0.0, cr), np.where(bad, 1.0, fo),
                        np.where(bad, 1.0, fr), device_out=True)
    nan = float("nan")
    badd = torch.from_numpy(bad).to("cuda") | none
    for k in ("restored_radprof", "fitted_restored", "wd"):
        met[k] = met[k].masked_fill(badd.reshape((-1,) + (1,) * (met[k].dim() - 1)), nan)
    t1.synchronize()
    sel_h = sel.cpu().numpy()
    status[kept] |= sel_h
    best_h = best.cpu().numpy()
    res = {nm: rows[:, j] for j, nm in enumerate(RESULT_KEYS[:5])}
    res.update(WD_RADIAL_PROFILE_DISTANCE=met["wd"], NUM_ITERS=nit,
               EXEC_TIME=torch.full((nk,), t0.elapsed_time(t1) * 1e-3 / nk, dtype=torch.float64,
                                    device="cuda"),
               best=best, scores=scores,
               beta_final=out["beta_final"][win].masked_fill(none, nan) if use_betadiv
               else torch.full((nk,), nan, dtype=torch.float64, device="cuda"),
               x=out["x"][win].masked_fill(none[:, None, None], nan),
               solver_status=out["counters"][:, 3].reshape(nk, K))
    if not device_out:
        res = _B.to_host(res)
        met = _B.to_host(met)
    res.update(kept=kept, status=status, metrics=met,
               best_beta=np.where(best_h >= 0, np.asarray(betas)[np.maximum(best_h, 0)], np.nan))
    return res
