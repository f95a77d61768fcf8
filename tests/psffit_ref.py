"""TEST INFRASTRUCTURE — numpy restatement of the PSF fit (DESIGN §3.14, P1 to
P8), the checker of bsgp_psf_fit_moments / bsgp_psf_fit_solve and
psf_calculate.fit_psf, and the synthetic frames the tests fit.

  fit(...)        the rules as the design states them: per-star moments, the
                  Kronecker assembly, the diagonally scaled Cholesky solve
                  (numpy.linalg.cholesky) and the clipping rounds.  The pixel
                  selection, the flux sum and every decision (status, used,
                  rounds) follow the device's order exactly; the sums of the
                  moments and of the assembly are numpy's, so coefficients
                  agree with the device's to rounding, not bit for bit.
  lstsq_fit(...)  numpy.linalg.lstsq on the explicit design matrix of the
                  stars a fit used: an independent solution of the same
                  least-squares problem.
  stamps(...)     the model at integer offsets about field positions, as
                  oracle/psf_oracle.py states it (held against it in
                  tests/test_psffit.py), vectorised.
  spread(...)     the yardstick of the GPU tests: the restatement rerun with
                  the pixels and stars in random order and every exp value
                  moved by -1, 0 or +1 ulp, its largest error kept.

Nothing here is imported by the product.
"""
import os

import numpy as np

GOLDEN_PSF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                          "psfccfbrd210048_1_1.bin.txt")
EPS = 2.0 ** -52
PARTIAL, BAD_POSITION, NO_OVERLAP, FEW_PIXELS, BAD_FLUX, BAD_WEIGHT, CLIPPED = 1, 2, 4, 8, 16, 32, 64
EXCLUDED = 2 | 4 | 8 | 16 | 32
SINGULAR = 128


def config(hw, W, H, ngauss=2, ldeg=2, sdeg=1, shape=None, sigma_inc=0.548, fitrad=None,
           origin=None):
    """The fixed part of a fit.  shape defaults to the golden file's."""
    if shape is None:
        import psf_oracle
        hdr, _ = psf_oracle.read_model(GOLDEN_PSF)
        shape = (hdr["cos"], hdr["sin"], hdr["ax"], hdr["ay"])
    ox, oy = (W / 2, H / 2) if origin is None else origin
    return dict(hw=hw, W=W, H=H, ngauss=ngauss, ldeg=ldeg, sdeg=sdeg, shape=tuple(shape),
                sigma_inc=sigma_inc, fitrad=float(hw) if fitrad is None else float(fitrad),
                origin=(float(ox), float(oy)), ncomp=ngauss * (ldeg + 1) * (ldeg + 2) // 2,
                nterm=(sdeg + 1) * (sdeg + 2) // 2)


def truth_coeffs(cfg):
    """Generating coefficients for a configuration, from the golden file's 36
    (two Gaussians, local degree 2, spatial degree 1): its leading spatial
    terms and Gaussians; a third Gaussian gets 0.3 times the first one's."""
    import psf_oracle
    _, c = psf_oracle.read_model(GOLDEN_PSF)
    c = np.asarray(c).reshape(3, 2, 6)
    assert cfg["ldeg"] == 2 and cfg["sdeg"] <= 1 and cfg["ngauss"] <= 3
    if cfg["ngauss"] == 3:
        c = np.concatenate([c, 0.3 * c[:, :1]], axis=1)
    return np.ascontiguousarray(c[:cfg["nterm"], :cfg["ngauss"]]).reshape(-1)


def basis(cfg, x, y, rng=None):
    """phi [len(x), ncomp] at real offsets (x, y): exp(rr_g) * x^m * y^n in
    calc_psf_pix's loop order and operation order.  With rng, every exp value
    is moved by -1, 0 or +1 ulp at random."""
    cs, sn, ax, ay = cfg["shape"]
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    x1 = cs * x - sn * y
    y1 = sn * x + cs * y
    rr = ax * x1 * x1 + ay * y1 * y1
    sig2 = cfg["sigma_inc"] * cfg["sigma_inc"]
    cols = []
    for _ in range(cfg["ngauss"]):
        f = np.exp(rr)
        if rng is not None:
            k = rng.integers(-1, 2, size=f.shape)
            f = np.where(k == 0, f, np.nextafter(f, np.where(k < 0, -np.inf, np.inf)))
        a1 = np.ones_like(x)
        for m in range(cfg["ldeg"] + 1):
            a2 = np.ones_like(x)
            for _n in range(cfg["ldeg"] - m + 1):
                cols.append(f * a1 * a2)
                a2 = a2 * y
            a1 = a1 * x
        rr = rr * sig2
    return np.stack(cols, axis=-1)


def spatial(cfg, px, py):
    """S [nterm]: (px - x_orig)^m (py - y_orig)^n in init_psf's loop order."""
    dx, dy = px - cfg["origin"][0], py - cfg["origin"][1]
    out = []
    a1 = 1.0
    for m in range(cfg["sdeg"] + 1):
        a2 = 1.0
        for _n in range(cfg["sdeg"] - m + 1):
            out.append(a1 * a2)
            a2 *= dy
        a1 *= dx
    return np.array(out)


def local_coeffs(cfg, coef, px, py):
    return spatial(cfg, px, py) @ np.asarray(coef).reshape(cfg["nterm"], cfg["ncomp"])


def stamps(cfg, coef, xy, hw=None):
    """[n, S, S] un-normalised stamps at integer offsets about the field
    positions xy: pixel (r, c) is the model at (x = c - hw, y = r - hw)."""
    hw = cfg["hw"] if hw is None else hw
    g = np.arange(-hw, hw + 1, dtype=np.float64)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    phi = basis(cfg, xx.ravel(), yy.ravel())
    S = 2 * hw + 1
    return np.stack([(phi @ local_coeffs(cfg, coef, x, y)).reshape(S, S) for x, y in xy])


def stamp_error(cfg, coef, ref_coef, xy):
    """Largest difference of the predicted stamps at xy, each over its reference's peak."""
    a, b = stamps(cfg, coef, xy), stamps(cfg, ref_coef, xy)
    return float(np.max(np.abs(a - b).reshape(len(xy), -1).max(axis=1) /
                        np.abs(b).reshape(len(xy), -1).max(axis=1)))


# ---------------------------------------------------------------- frames
def star_grid(n, W, H, hw, rng):
    """n sub-pixel positions on a jittered grid whose pitch exceeds 2 hw + 1, so
    that no fit box holds a neighbour and every box lies inside the frame."""
    g = int(np.ceil(np.sqrt(n)))
    px, py = W / g, H / g
    assert min(px, py) > 2 * hw + 2, "the grid pitch must exceed the box"
    cells = [(i, j) for j in range(g) for i in range(g)][:n]
    jx, jy = (px - (2 * hw + 2)) / 2, (py - (2 * hw + 2)) / 2
    return np.array([[(i + 0.5) * px - 0.5 + rng.uniform(-jx, jx),
                      (j + 0.5) * py - 0.5 + rng.uniform(-jy, jy)] for i, j in cells])


def add_star(img, cfg, coef, x, y, flux, at=None):
    """Add flux * model to img over the (2 hw + 3)^2 pixels about (x, y), the
    model being the one of field position `at` (default (x, y))."""
    H, W = img.shape
    hw = cfg["hw"] + 1
    ic, ir = int(np.floor(x + 0.5)), int(np.floor(y + 0.5))
    r = np.arange(max(0, ir - hw), min(H, ir + hw + 1))
    c = np.arange(max(0, ic - hw), min(W, ic + hw + 1))
    if len(r) == 0 or len(c) == 0:
        return
    rr, cc = np.meshgrid(r, c, indexing="ij")
    ax, ay = (x, y) if at is None else at
    phi = basis(cfg, cc.ravel() - x, rr.ravel() - y)
    img[rr, cc] += flux * (phi @ local_coeffs(cfg, coef, ax, ay)).reshape(rr.shape)


def make_frame(cfg, nstars, seed, sky=0.0, noise=0.0, xy=None):
    """(image float64, xy [n, 2], flux [n], truth coefficients): stars of the
    truth model at sub-pixel positions with fluxes over two decades, on a
    constant sky, plus Gaussian noise of sigma = noise * each star's peak."""
    rng = np.random.default_rng(seed)
    W, H = cfg["W"], cfg["H"]
    coef = truth_coeffs(cfg)
    xy = star_grid(nstars, W, H, cfg["hw"], rng) if xy is None else np.asarray(xy, dtype=np.float64)
    flux = 10.0 ** rng.uniform(2.0, 4.0, size=len(xy))
    img = np.full((H, W), float(sky))
    sigma = np.zeros((H, W))
    for (x, y), f in zip(xy, flux):
        if not (np.isfinite(x) and np.isfinite(y)):
            continue
        one = np.zeros((H, W))
        add_star(one, cfg, coef, x, y, f)
        img += one
        sigma = np.maximum(sigma, noise * one.max() * (one != 0))
    if noise:
        img = img + sigma * rng.standard_normal((H, W))
    return img, xy, flux, coef


# ---------------------------------------------------------------- the fit
def star_pixels(cfg, image, px, py, sky=0.0, mask=None, sat_level=None):
    """P1: (status, rows, cols, d) of a star: its fit pixels in row-major
    order and their values minus the sky (float64)."""
    H, W = image.shape
    hw = cfg["hw"]
    none = np.zeros(0, dtype=np.int64)
    if not (np.isfinite(px) and np.isfinite(py)):
        return BAD_POSITION, none, none, np.zeros(0)
    ic = int(np.clip(np.floor(px + 0.5), -2.0 ** 30, 2.0 ** 30))
    ir = int(np.clip(np.floor(py + 0.5), -2.0 ** 30, 2.0 ** 30))
    if ic + hw < 0 or ic - hw >= W or ir + hw < 0 or ir - hw >= H:
        return NO_OVERLAP, none, none, np.zeros(0)
    status = PARTIAL if (ic - hw < 0 or ic + hw >= W or ir - hw < 0 or ir + hw >= H) else 0
    r = np.arange(max(0, ir - hw), min(H, ir + hw + 1))
    c = np.arange(max(0, ic - hw), min(W, ic + hw + 1))
    rr, cc = (a.ravel() for a in np.meshgrid(r, c, indexing="ij"))
    x, y = cc - px, rr - py
    val = image[rr, cc].astype(np.float64)
    s = sky[rr, cc] if np.ndim(sky) == 2 else float(sky)
    with np.errstate(invalid="ignore"):
        d = val - s
        ok = (x * x + y * y <= cfg["fitrad"] * cfg["fitrad"]) & np.isfinite(d)
        if mask is not None:
            ok &= mask[rr, cc] == 0
        if sat_level is not None:
            ok &= ~(val >= sat_level)
    return status, rr[ok], cc[ok], d[ok]


def moments(cfg, image, xy, flux=None, sky=0.0, mask=None, sat_level=None, rng=None):
    """P1 to P3 for every star: a list of dicts with status, npix, flux, the
    design rows phi and observations v, and the moments G (full), h, vv."""
    out = []
    for s, (px, py) in enumerate(xy):
        sk = sky[s] if np.ndim(sky) == 1 else sky
        status, rr, cc, d = star_pixels(cfg, image, px, py, sk, mask, sat_level)
        nc = cfg["ncomp"]
        st = dict(status=status, npix=0, flux=np.nan, px=px, py=py, G=np.zeros((nc, nc)),
                  h=np.zeros(nc), vv=0.0, phi=np.zeros((0, nc)), v=np.zeros(0))
        out.append(st)
        if status & EXCLUDED:
            if flux is not None:
                st["flux"] = float(flux[s])
            continue
        # the flux: given, or the sum in pixel order (cumsum adds one by one)
        F = float(flux[s]) if flux is not None else (float(np.cumsum(d)[-1]) if len(d) else 0.0)
        st["flux"], st["npix"] = F, len(d)
        if not (F > 0.0 and np.isfinite(F)):
            st["status"] |= BAD_FLUX
            if flux is not None:
                st["npix"] = 0  # refused before the pixels are read
            continue
        if len(d) < nc:
            st["status"] |= FEW_PIXELS
            continue
        phi = basis(cfg, cc - px, rr - py, rng)
        v = d / F
        if rng is not None:
            p = rng.permutation(len(v))
            phi, v = phi[p], v[p]
        st.update(phi=phi, v=v, G=phi.T @ phi, h=phi.T @ v, vv=float(v @ v))
    return out


def solve(cfg, stars, active, weights=None):
    """P4 to P6: coefficients [P] from the moments of the active stars, or
    None when a scaled pivot is not above P * 2^-52."""
    nc, nt = cfg["ncomp"], cfg["nterm"]
    P = nc * nt
    N, b = np.zeros((P, P)), np.zeros(P)
    for s in active:
        st = stars[s]
        w = 1.0 if weights is None else float(weights[s])
        S = spatial(cfg, st["px"], st["py"])
        N += np.kron(w * np.outer(S, S), st["G"])
        b += np.kron(w * S, st["h"])
    dg = np.diag(N).copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        A = N / np.sqrt(np.outer(dg, dg))
        d = np.sqrt(dg)
    if not np.all(np.isfinite(A)):
        return None
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    if np.any(np.diag(L) ** 2 <= P * EPS):
        return None
    z = np.linalg.solve(L.T, np.linalg.solve(L, b / d))
    return z / d


def residuals(cfg, stars, active, coef):
    """P7: {star: (rss, rms)} from the moments."""
    out = {}
    for s in active:
        st = stars[s]
        c = local_coeffs(cfg, coef, st["px"], st["py"])
        rss = max(0.0, (st["vv"] - 2.0 * (c @ st["h"])) + c @ (st["G"] @ c))
        out[s] = (rss, np.sqrt(rss / st["npix"]))
    return out


def fit(cfg, image, xy, flux=None, sky=0.0, mask=None, sat_level=None, weights=None, niter=0,
        nsig=2.0, min_stars=0, rng=None, trace=None):
    """The whole estimator.  Returns a dict: coef ([P], NaN when singular),
    used, status, rms, flux, npix (per star), rounds, frame_status.  `trace`,
    a list, receives per clipping round (threshold, {star: rms}, dropped)."""
    stars = moments(cfg, image, xy, flux, sky, mask, sat_level, rng)
    n = len(stars)
    status = np.array([st["status"] for st in stars], dtype=np.int32).reshape(n)
    if weights is not None:
        for s in range(n):
            w = float(weights[s])
            if not (status[s] & EXCLUDED) and not (w > 0.0 and np.isfinite(w)):
                status[s] |= BAD_WEIGHT
    active = [s for s in range(n) if not (status[s] & EXCLUDED)]
    rms = np.full(n, np.nan)
    rounds, fstatus = 0, 0
    P = cfg["ncomp"] * cfg["nterm"]
    coef = np.full(P, np.nan)
    while True:
        order = list(active)
        if rng is not None:
            rng.shuffle(order)
        c = solve(cfg, stars, order, weights)
        if c is None:
            fstatus, coef, rms[:] = SINGULAR, np.full(P, np.nan), np.nan
            break
        coef = c
        res = residuals(cfg, stars, active, coef)
        for s, (_, r) in res.items():
            rms[s] = r
        if rounds >= niter or not active:
            break
        r_act = np.array([res[s][1] for s in active])
        med = np.median(r_act)
        mad = np.median(np.abs(r_act - med))
        thr = med + nsig * 1.4826 * mad
        drop = [s for s in active
                if res[s][1] > thr and res[s][0] > 4096.0 * EPS * stars[s]["vv"]]
        if trace is not None:
            trace.append((thr, {s: res[s][1] for s in active}, drop))
        if not drop or len(active) - len(drop) < max(cfg["nterm"], min_stars):
            break
        for s in drop:
            status[s] |= CLIPPED
        active = [s for s in active if s not in drop]
        rounds += 1
    used = np.zeros(n, dtype=bool)
    used[active] = True
    return dict(coef=coef, used=used, status=status, rms=rms, rounds=rounds, frame_status=fstatus,
                flux=np.array([st["flux"] for st in stars]).reshape(n),
                npix=np.array([st["npix"] for st in stars], dtype=np.int32).reshape(n), stars=stars)


def lstsq_fit(cfg, res, weights=None):
    """numpy.linalg.lstsq on the explicit design matrix (rows S (x) phi, times
    sqrt(w)) of the stars a fit used; columns scaled to unit norm."""
    rows, obs = [], []
    for s in np.flatnonzero(res["used"]):
        st = res["stars"][s]
        w = 1.0 if weights is None else float(weights[s])
        S = spatial(cfg, st["px"], st["py"])
        rows.append(np.sqrt(w) * np.kron(S[None, :], st["phi"]))
        obs.append(np.sqrt(w) * st["v"])
    A, v = np.concatenate(rows), np.concatenate(obs)
    scale = np.linalg.norm(A, axis=0)
    return np.linalg.lstsq(A / scale, v, rcond=None)[0] / scale


def spread(cfg, ref_coef, xy_eval, runs=32, seed=1234, **fit_args):
    """The largest stamp_error against ref_coef of `runs` reruns of the
    restatement with permuted pixels and stars and +-1 ulp on every exp."""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(runs):
        r = fit(cfg, rng=rng, **fit_args)
        worst = max(worst, stamp_error(cfg, r["coef"], ref_coef, xy_eval))
    return worst


# ---------------------------------------------------------------- the tests' cases
SKY = 37.5
# name: (hw, frame size, stars, ngauss, sdeg, seed)
RECOVERY = {
    "hw4_3stars": (4, 40, 3, 2, 1, 11),     # three non-collinear stars: the spatial part is exactly determined
    "hw6_16stars": (6, 80, 16, 2, 1, 12),
    "hw15_16stars": (15, 450, 16, 2, 1, 13),  # a 961-pixel box: no multiple of a chunk
    "g1_s0_1star": (6, 40, 1, 1, 0, 14),
    "g3_p54": (6, 80, 16, 3, 1, 15),
}


def recovery_case(name):
    """Noise-free stars on a constant sky, flux and sky known: (cfg, fit arguments, truth)."""
    hw, size, n, ngauss, sdeg, seed = RECOVERY[name]
    cfg = config(hw, size, size, ngauss=ngauss, sdeg=sdeg)
    img, xy, flux, coef = make_frame(cfg, n, seed, sky=SKY)
    return cfg, dict(image=img, xy=xy, flux=flux, sky=SKY), coef


def sky_map(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return SKY + 0.05 * xx - 0.03 * yy


def noisy_case(seed=21, hw=6, size=80, n=16):
    """Test 2: a float32 frame with noise of 1e-3 of each star's peak on a sky
    map, the flux left to the fit."""
    cfg = config(hw, size, size)
    img, xy, flux, coef = make_frame(cfg, n, seed, sky=0.0, noise=1e-3)
    sky = sky_map(size, size)
    return cfg, dict(image=(img + sky).astype(np.float32), xy=xy, flux=None, sky=sky), coef


def geometry_case(seed=31):
    """Test 3: nine grid stars on an 80^2 frame, of which star 0 sits at the
    frame's edge (box partly outside), star 4 has masked and NaN pixels in its
    box and star 8 is bright enough for its core to reach sat_level; star 9
    lies outside the frame and star 10 has a NaN position."""
    cfg = config(6, 80, 80)
    rng = np.random.default_rng(seed)
    coef = truth_coeffs(cfg)
    xy = star_grid(9, 80, 80, 6, rng)
    xy[0] = (1.7, 12.6)
    xy = np.concatenate([xy, [[-20.0, 40.0], [np.nan, 30.0]]])
    flux = 10.0 ** rng.uniform(2.0, 3.0, size=len(xy))
    flux[8] = 3e4
    img = np.zeros((80, 80))
    for (x, y), f in zip(xy[:9], flux[:9]):
        add_star(img, cfg, coef, x, y, f)
    peak = [img[int(np.floor(y + 0.5)), int(np.floor(x + 0.5))] for x, y in xy[:9]]
    sat = 0.5 * peak[8]
    assert max(peak[:8]) < 0.5 * sat
    img = img + 1e-3 * max(peak[:8]) * rng.standard_normal(img.shape)
    mask = np.zeros((80, 80), dtype=bool)
    c4, r4 = int(np.floor(xy[4, 0] + 0.5)), int(np.floor(xy[4, 1] + 0.5))
    mask[r4 - 2, c4 - 3:c4 + 2] = True
    img[r4 + 3, c4 + 1] = np.nan
    img[r4, c4 - 4] = np.inf
    return cfg, dict(image=img + SKY, xy=xy, flux=flux, sky=SKY, mask=mask, sat_level=sat + SKY), coef


def clip_case(seed=28, nsig=10.0, bad=(5, 10)):
    """Test 4: the noisy 16-star case with a neighbour of 0.3 x flux 3 px off
    the centre of two stars; niter = 3."""
    cfg, args, coef = noisy_case(seed)
    img = args["image"].astype(np.float64)
    _, xy, flux, _ = make_frame(cfg, 16, seed, sky=0.0, noise=1e-3)
    for s in bad:
        add_star(img, cfg, coef, xy[s, 0] + 3.0, xy[s, 1], 0.3 * flux[s], at=tuple(xy[s]))
    args = dict(args, image=img.astype(np.float32), niter=3, nsig=nsig)
    return cfg, args, coef, bad


def measure_spreads(runs=32):
    """{case: the largest error of `runs` perturbed reruns}: the yardsticks that
    tests/test_gpu_psffit.py records (its bounds are 4 times these).  Test 1
    measures against the truth, tests 2 to 4 against lstsq_fit."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    out = {}
    for name in RECOVERY:
        cfg, args, truth = recovery_case(name)
        out[name] = spread(cfg, truth, args["xy"], runs, **args)
    for name, case in (("noisy", noisy_case), ("geometry", geometry_case), ("clip", clip_case)):
        cfg, args, *_ = case()
        res = fit(cfg, **args)
        xy = args["xy"][np.isfinite(args["xy"]).all(axis=1) & (res["status"] & EXCLUDED == 0)]
        out[name] = spread(cfg, lstsq_fit(cfg, res), xy, runs, **args)
    return out


if __name__ == "__main__":
    for k, v in measure_spreads().items():
        print(f"{k:14s} spread {v:.3g}  bound {4 * v:.3g}")
