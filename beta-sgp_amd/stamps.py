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

``center`` is ``(c0, c1)`` with ``c0`` measured along the rows (axis 0), as
the reference's ``np.indices`` order has it; the reference passes
``(xcentroid, ycentroid)`` there, and that quirk is kept: pass what the
reference passes to get what it gets.
"""
import numpy as np

import _bsgp as _B

MAX_PIXELS = 16384  # H * W of one stamp
MAX_BINS = 256      # radial bins, profile length, sample length


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
