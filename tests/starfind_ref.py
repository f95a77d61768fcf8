"""Plain-numpy restatement of star finding (include/bsgp.h and DESIGN §3.15,
F1 to F10): what ``starfind.find_stars`` and ``starfind.select_psf_stars``
compute on the device.  tests/golden/make_golden_starfind.py writes
tests/golden/starfind_cases.npz with it.

Device and restatement add the same float64 terms in the same order wherever
the rule fixes an order (F3's sums over the support, F7's sums by rows), so the
maps, the candidate list and every column that follows from a given sky are
equal bit for bit.  The sky's mean and standard deviation differ by summation
order, as the local background's do; ``sky`` returns the derived bar."""
import numpy as np

BAD_FLUX, OFF_CENTRE, FEW_SKY, SKY_OVER_CAP = 1, 2, 4, 8
REJECTED = BAD_FLUX | OFF_CENTRE | FEW_SKY | SKY_OVER_CAP
OVER_CAP = 16
MAX_R, MAX_STARS, MAX_SKY, MIN_SKY = 15, 16384, 8192, 10
SKY_SIGMA, SKY_MAXITERS = 3.0, 10
FWHM_TO_SIGMA = 0.42466090014400953  # astropy's gaussian_fwhm_to_sigma: 1 / (2 sqrt(2 ln 2))
SIGMA_TO_FWHM = 2.3548200450309493   # 2 sqrt(2 ln 2)
U = 2.0 ** -53
FCOLS = ("x", "y", "flux", "bkg", "peak", "corr", "amp", "fwhm")


def template(fwhm, aprad=1.2):
    """F1: dict(R, rap, n, dy [n], dx [n], halfw [2R + 1], t [n], tt)."""
    rap = aprad * fwhm
    R = int(np.floor(rap))
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    r2 = (dx * dx + dy * dy).astype(np.float64)
    inside = r2 <= rap * rap
    dy, dx, r2 = dy[inside], dx[inside], r2[inside]  # row-major
    sigma = fwhm * FWHM_TO_SIGMA
    g = np.exp(-r2 / (2.0 * sigma * sigma))
    t = g - g.sum() / len(g)
    halfw = np.array([dx[dy == r].max() for r in range(-R, R + 1)], dtype=np.int32)
    return dict(R=R, rap=rap, n=len(t), dy=dy, dx=dx, halfw=halfw, t=t, tt=float(np.sum(t * t)))


def maps(image, tp, mask=None):
    """F2, F3: (corr, amp, st) [H, W] float64, NaN where p is not valid."""
    I = np.asarray(image).astype(np.float64)
    H, W = I.shape
    R, n = tp["R"], tp["n"]
    corr, amp, stm = (np.full((H, W), np.nan) for _ in range(3))
    if H < 2 * R + 1 or W < 2 * R + 1:
        return corr, amp, stm
    h, w = H - 2 * R, W - 2 * R
    badpix = ~np.isfinite(I)
    if mask is not None:
        badpix |= np.asarray(mask) != 0
    s1, s2, st = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    bad = np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        for k in range(n):
            ys, xs = R + tp["dy"][k], R + tp["dx"][k]
            v = I[ys:ys + h, xs:xs + w]
            bad |= badpix[ys:ys + h, xs:xs + w]
            s1 = s1 + v
            s2 = s2 + v * v
            st = st + tp["t"][k] * v
        var = s2 - s1 * s1 / float(n)
        a = st / tp["tt"]
        c = np.where(var > 0.0, st / np.sqrt(tp["tt"] * var), 0.0)
    for out, val in ((corr, c), (amp, a), (stm, st)):
        out[R:H - R, R:W - R] = np.where(bad, np.nan, val)
    return corr, amp, stm


def candidates(corr, amp, st, noise, tt, c_min=0.4, thresh=2.0, peak_hw=1):
    """F4, F5: (ir, ic) of the candidates in raster order, and the margins of
    the decisions: the smallest |corr - c_min| and the smallest relative
    distance of st to its threshold over the valid pixels."""
    H, W = amp.shape
    valid = ~np.isnan(amp)
    thr = (thresh * np.asarray(noise, dtype=np.float64)) * np.sqrt(tt)
    with np.errstate(all="ignore"):
        ok = valid & (corr >= c_min) & (st >= thr)
        m_corr = np.min(np.abs(corr[valid] - c_min)) if valid.any() else np.inf
        rel = np.abs(st - thr) / np.abs(thr)
        m_sig = np.min(rel[valid & np.isfinite(rel)]) if valid.any() else np.inf
        p = peak_hw
        pad = np.full((H + 2 * p, W + 2 * p), np.nan)
        pad[p:p + H, p:p + W] = amp
        for wy in range(-p, p + 1):
            for wx in range(-p, p + 1):
                if wy == 0 and wx == 0:
                    continue
                u = pad[p + wy:p + wy + H, p + wx:p + wx + W]
                earlier = wy < 0 or (wy == 0 and wx < 0)
                ok &= np.isnan(u) | ((amp > u) if earlier else (amp >= u))
    ir, ic = np.nonzero(ok)  # row-major: raster order
    return ir.astype(np.int32), ic.astype(np.int32), dict(corr=float(m_corr), sig=float(m_sig))


def annulus_values(image, ic, ir, anrad1, anrad2, mask=None, sat_level=None):
    """F6: the float64 values of the sky annulus about (ic, ir), sorted."""
    I = np.asarray(image)
    H, W = I.shape
    dy = (np.arange(H) - ir)[:, None]
    dx = (np.arange(W) - ic)[None, :]
    d2 = (dx * dx + dy * dy).astype(np.float64)
    m = (d2 >= anrad1 * anrad1) & (d2 <= anrad2 * anrad2)
    if mask is not None:
        m &= np.asarray(mask) == 0
    v = I[m].astype(np.float64)
    v = v[np.isfinite(v)]
    if sat_level is not None:
        v = v[v < sat_level]
    return np.sort(v)


def clip_sorted(s, sigma=SKY_SIGMA, maxiters=SKY_MAXITERS):
    """§3.8's L4 on the sorted values s: (lo, hi, iterations, median, mean,
    std, margin), margin the smallest relative distance of a value to a
    clipping bound over the iterations."""
    lo, hi, it, more, margin = 0, len(s), 0, maxiters > 0, np.inf
    while True:
        v, n = s[lo:hi], hi - lo
        med = v[n // 2] if n & 1 else (v[n // 2 - 1] + v[n // 2]) / 2.0
        mean = v.sum() / n
        sd = np.sqrt(((v - mean) ** 2).sum() / n)
        if not more:
            break
        lb, ub = med - sd * sigma, med + sd * sigma
        if sd > 0:
            dist = min(np.min(np.abs(v - lb)), np.min(np.abs(v - ub)))
            margin = min(margin, dist / max(abs(lb), abs(ub)))
        nlo, nhi = lo + np.searchsorted(v, lb, "left"), lo + np.searchsorted(v, ub, "right")
        it += 1
        if nhi <= nlo:
            return int(nlo), int(nlo), it, np.nan, np.nan, np.nan, margin
        changed = (nlo, nhi) != (lo, hi)
        lo, hi = int(nlo), int(nhi)
        if not changed:
            break
        more = it < maxiters
    return lo, hi, it, float(med), float(mean), float(sd), margin


def sky(image, ic, ir, anrad1=20.0, anrad2=25.0, bkg_alg="mode", mask=None, sat_level=None):
    """F6: dict(bkg, status, nsky, nsurv, bar, margin, branch).  bar bounds
    what another summation order of the survivors does to bkg (tests/
    localbkg_ref.py's): 0 for the median, which is exact; branch is
    | |mean - median| / std - 0.3 | for the mode (inf where it does not decide)."""
    s = annulus_values(image, ic, ir, anrad1, anrad2, mask, sat_level)
    out = dict(bkg=np.nan, status=0, nsky=len(s), nsurv=0, bar=0.0, margin=np.inf, branch=np.inf)
    if len(s) > MAX_SKY:
        out["status"] = SKY_OVER_CAP
        return out
    if len(s) < MIN_SKY:
        out["status"] = FEW_SKY
        return out
    lo, hi, _, med, mean, sd, margin = clip_sorted(s)
    out.update(nsurv=hi - lo, margin=margin)
    if hi <= lo:
        return out
    sabs = np.abs(s[lo:hi]).sum()
    mean_bar = 2 * U * sabs + U * abs(mean)
    if bkg_alg == "median":
        out["bkg"] = med
    elif bkg_alg == "mean":
        out.update(bkg=mean, bar=mean_bar)
    elif sd == 0:
        out.update(bkg=mean, bar=mean_bar)
    else:
        ratio = abs(mean - med) / sd
        out["branch"] = abs(ratio - 0.3)
        if ratio < 0.3:
            out.update(bkg=2.5 * med - 1.5 * mean, bar=1.5 * mean_bar + 4 * U * (abs(med) + abs(mean)))
        else:
            out["bkg"] = med
    return out


def measure(image, ic, ir, bkg, tp, sat_level=None, dxy=1.0):
    """F7, F8 (without the sky's bits) of one star with the sky ``bkg``, in
    Python floats: every operation a rounded float64 one, in the rule's order."""
    I = np.asarray(image)
    R, bkg = tp["R"], float(bkg)
    S = [0.0] * 6
    mx, bx, by, nsat = 0.0, 0, 0, 0
    with np.errstate(all="ignore"):
        for r in range(2 * R + 1):
            dy, w = r - R, int(tp["halfw"][r])
            row = [0.0] * 6
            rmx, rarg = 0.0, 0
            for dx in range(-w, w + 1):
                v = float(I[ir + dy, ic + dx])
                J = v - bkg
                row[0] += J
                row[1] += float(dx) * J
                row[2] += float(dy) * J
                row[3] += float(dx * dx) * J
                row[4] += float(dy * dy) * J
                row[5] += float(dx * dy) * J
                if dx == -w or v > rmx:
                    rmx, rarg = v, dx
                if sat_level is not None and v >= sat_level:
                    nsat += 1
            for q in range(6):
                S[q] += row[q]
            if r == 0 or rmx > mx:
                mx, bx, by = rmx, rarg, dy
        S = np.array(S)  # numpy scalars: a division by zero gives inf / NaN, as on the device
        F = S[0]
        mxx, myy = S[1] / F, S[2] / F
        x, y = float(ic) + mxx, float(ir) + myy
        arg = ((S[3] / F - mxx * mxx) + (S[4] / F - myy * myy)) / 2.0
        fwhm = SIGMA_TO_FWHM * np.sqrt(arg) if arg > 0.0 else np.nan
        status = 0
        if not (np.isfinite(F) and F > 0.0):
            status |= BAD_FLUX
        ex, ey = float(ic + bx) - x, float(ir + by) - y
        d2 = ex * ex + ey * ey
        if d2 > dxy * dxy:
            status |= OFF_CENTRE
    return dict(x=float(x), y=float(y), flux=float(F), bkg=bkg, peak=float(mx - bkg),
                fwhm=float(fwhm), nsat=nsat, status=status, d2=float(d2))


def find_stars(image, fwhm, noise, mask=None, sat_level=None, c_min=0.4, aprad=1.2, anrad1=20.0,
               anrad2=25.0, thresh=2.0, dxy=1.0, bkg_alg="mode", peak_hw=1, max_stars=MAX_STARS,
               tp=None, bkg=None):
    """F1 to F8 of one frame.  ``bkg``: per-candidate skies to measure with
    instead of F6's (the device's, for the columns that follow from them).
    Returns a dict: the columns as arrays over the candidates, ``ic``, ``ir``,
    ``nsat``, ``status``, ``frame_status``, ``corr_map``, ``amp_map``, the
    sky's ``bar`` / ``margin`` / ``branch`` / ``nsky``, ``d2`` and ``margins``."""
    tp = template(fwhm, aprad) if tp is None else tp
    corr, amp, st = maps(image, tp, mask)
    ir, ic, margins = candidates(corr, amp, st, noise, tp["tt"], c_min, thresh, peak_hw)
    frame_status = OVER_CAP if len(ir) > max_stars else 0
    ir, ic = ir[:max_stars], ic[:max_stars]
    n = len(ir)
    out = {k: np.full(n, np.nan) for k in FCOLS + ("bar", "margin", "branch", "d2")}
    out.update(ic=ic, ir=ir, nsat=np.zeros(n, np.int32), status=np.zeros(n, np.int32),
               nsky=np.zeros(n, np.int32), frame_status=frame_status, corr_map=corr, amp_map=amp,
               margins=margins, template=tp)
    for k in range(n):
        sk = sky(image, ic[k], ir[k], anrad1, anrad2, bkg_alg, mask, sat_level)
        b = sk["bkg"] if bkg is None else bkg[k]
        m = measure(image, ic[k], ir[k], b, tp, sat_level, dxy)
        for c in ("x", "y", "flux", "bkg", "peak", "fwhm", "d2"):
            out[c][k] = m[c]
        out["corr"][k], out["amp"][k] = corr[ir[k], ic[k]], amp[ir[k], ic[k]]
        out["nsat"][k], out["status"][k] = m["nsat"], m["status"] | sk["status"]
        out["nsky"][k] = sk["nsky"]
        for c in ("bar", "margin", "branch"):
            out[c][k] = sk[c]
    return out


def select_psf_stars(x, y, flux, peak, nsat, status, shape, fwhm=None, hw=15, min_flux=100.0,
                     max_peak=None, rat_thresh=0.2, iso_radius=None, npsf_max=100):
    """F9 on the columns: (indices in rank order, eligible, rank)."""
    x, y, flux, peak = (np.asarray(v, dtype=np.float64) for v in (x, y, flux, peak))
    nsat, status = np.asarray(nsat), np.asarray(status)
    H, W = shape
    n = len(x)
    iso_radius = 3.0 * fwhm if iso_radius is None else iso_radius
    kept = (status & REJECTED) == 0
    with np.errstate(all="ignore"):
        pre = kept & (flux >= min_flux) & (nsat == 0)
        if max_peak is not None:
            pre &= peak <= max_peak
        cx, cy = np.floor(x + 0.5), np.floor(y + 0.5)
        pre &= (cx - hw >= 0) & (cx + hw < W) & (cy - hw >= 0) & (cy + hw < H)
        dx, dy = x[None, :] - x[:, None], y[None, :] - y[:, None]  # [s, t] = t - s
        near = dx * dx + dy * dy <= iso_radius * iso_radius
        rival = kept[None, :] & (flux[None, :] >= rat_thresh * flux[:, None]) & near
        rival &= ~np.eye(n, dtype=bool)
        eligible = pre & ~rival.any(axis=1)
        idx = np.arange(n)
        ahead = eligible[None, :] & ((flux[None, :] > flux[:, None]) |
                                     ((flux[None, :] == flux[:, None]) & (idx[None, :] < idx[:, None])))
    rank = np.where(eligible, ahead.sum(axis=1), -1).astype(np.int32)
    sel = np.flatnonzero(eligible & (rank < npsf_max))
    return sel[np.argsort(rank[sel])], eligible, rank


def seeing(cols, shape, min_fwhm=2.6, max_fwhm=10.0, min_peak=500.0, max_peak=2e4, margin=5):
    """fwhmm's role: the median fwhm of the kept stars inside fwhmm.par's limits."""
    H, W = shape
    with np.errstate(all="ignore"):
        ok = ((cols["status"] & REJECTED) == 0) & (cols["fwhm"] >= min_fwhm) & \
            (cols["fwhm"] <= max_fwhm) & (cols["peak"] >= min_peak) & (cols["peak"] <= max_peak) & \
            (cols["x"] >= margin) & (cols["x"] <= W - 1 - margin) & \
            (cols["y"] >= margin) & (cols["y"] <= H - 1 - margin)
    return float(np.median(cols["fwhm"][ok])) if ok.any() else float("nan")
