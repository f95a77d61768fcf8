"""Generate tests/golden/bkg2d_cases.npz: inputs and expected outputs of the
device background estimator (beta-sgp_amd/background.py).

photutils is not available, so the expected values come from the parts it is
built from: sigma clipping through ``astropy.stats.SigmaClip`` (astropy 4.3.1),
the mesh median filter through ``scipy.ndimage.generic_filter`` and the zoom
through ``scipy.ndimage.zoom``; the fill of excluded boxes, which DESIGN §3.7
defines itself, is restated here in plain numpy.  Run from the repository
root with the interpreter that has astropy 4.3.1 and scipy (python 3.9, the
one make_golden.py's ``linear`` / ``app`` modes use):

    PYTHONDONTWRITEBYTECODE=1 python3.9 tests/golden/make_golden_bkg.py

The generator asserts, for every box and every clipping iteration of every
case, that no pixel lies within MARGIN (relative to the larger bound's
magnitude) of a clipping bound, so that a 1e-12 difference in a standard
deviation cannot change which pixels survive (exempt where the std is 0:
there the inclusive bounds keep every pixel).  The synthetic cases take the
first seed that satisfies it.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402

# astropy 4.3.1 on numpy 1.26 needs these removed numpy aliases (as make_golden.py)
if not hasattr(np, "asscalar"):
    np.asscalar = lambda a: a.item()
if not hasattr(np, "alen"):
    np.alen = len
from astropy.stats import SigmaClip  # noqa: E402
from scipy import ndimage  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-9


class MarginError(AssertionError):
    pass


def clip_box(v, sigma, maxiters):
    """Survivors of astropy's sigma clipping of the 1-D float64 values v, the
    iterations it ran (the last one may remove nothing) and the smallest
    relative distance of a pixel to a clipping bound over those iterations."""
    def run(k):
        if k == 0:
            return v
        out = SigmaClip(sigma=sigma, maxiters=k, cenfunc="median", stdfunc="std")(v, masked=False)
        return out[np.isfinite(out)]

    surv, iters, margin = v, 0, np.inf
    for k in range(1, maxiters + 1):
        c, s = np.median(surv), np.std(surv)
        lb, ub = c - sigma * s, c + sigma * s
        if s > 0:
            d = min(np.min(np.abs(surv - lb)), np.min(np.abs(surv - ub)))
            margin = min(margin, d / max(abs(lb), abs(ub)))
        nxt = run(k)
        iters = k
        if len(nxt) == len(surv):
            break
        surv = nxt
    assert len(run(maxiters)) == len(surv)
    return surv, iters, margin


def fill_excluded(mesh, excl):
    """Inverse-distance (power 1) mean of the up-to-10 nearest kept cells,
    nearest first, ties in row-major order."""
    ny, nx = mesh.shape
    kept = [(y, x) for y in range(ny) for x in range(nx) if not excl[y, x]]
    out = mesh.copy()
    for y in range(ny):
        for x in range(nx):
            if not excl[y, x]:
                continue
            d2 = [(ky - y) ** 2 + (kx - x) ** 2 for ky, kx in kept]
            order = sorted(range(len(kept)), key=lambda k: (d2[k], k))[:10]
            sw = swv = 0.0
            for k in order:
                w = 1.0 / np.sqrt(float(d2[k]))
                sw += w
                swv += w * mesh[kept[k]]
            out[y, x] = swv / sw
    return out


def reference(data, box, filt, sigma=3.0, maxiters=10, exclude_percentile=10.0, clip=True,
              mask=None):
    d = np.asarray(data).astype(np.float64)
    H, W = d.shape
    bh, bw = box
    ny, nx = -(-H // bh), -(-W // bw)
    pad = np.full((ny * bh, nx * bw), np.nan)
    pad[:H, :W] = np.where(np.isfinite(d), d, np.nan)
    if mask is not None:
        pad[:H, :W][np.asarray(mask, bool)] = np.nan
    boxes = pad.reshape(ny, bh, nx, bw).swapaxes(1, 2).reshape(ny, nx, bh * bw)
    ninvalid = np.isnan(boxes).sum(axis=2)
    excl = (ninvalid > exclude_percentile / 100.0 * (bh * bw)) | (ninvalid == bh * bw)
    if excl.all():
        raise ValueError("every box excluded")
    med = np.full((ny, nx), np.nan)
    std = np.full((ny, nx), np.nan)
    nsurv = np.zeros((ny, nx), np.int32)
    niter = np.zeros((ny, nx), np.int32)
    margin = np.inf
    for j in range(ny):
        for i in range(nx):
            if excl[j, i]:
                continue
            v = boxes[j, i][~np.isnan(boxes[j, i])]
            surv, it, mg = clip_box(v, sigma, maxiters)
            margin = min(margin, mg)
            med[j, i], std[j, i] = np.median(surv), np.std(surv)
            nsurv[j, i], niter[j, i] = len(surv), it
    if margin < MARGIN:
        raise MarginError(f"a pixel lies within {margin:.2e} of a clipping bound")
    out = dict(excl=excl, raw_med=med, raw_std=std, nsurv=nsurv, niter=niter, margin=margin)
    # cells of the filtered mesh that the filter fed only unfilled values
    out["pure"] = ndimage.maximum_filter(excl.astype(np.uint8), size=filt, mode="constant",
                                         cval=0) == 0
    for name, m in (("bkg", med), ("rms", std)):
        filled = fill_excluded(m, excl)
        f = ndimage.generic_filter(filled, np.nanmedian, size=filt, mode="constant", cval=np.nan)
        z = ndimage.zoom(f, (bh, bw), order=3, mode="reflect", grid_mode=True)
        assert z.shape == (ny * bh, nx * bw)
        out[name + "_unclipped_range"] = np.array([z[:H, :W].min(), z[:H, :W].max()])
        if clip:
            z = np.clip(z, f.min(), f.max())
        out[name + "_filled"], out[name + "_mesh"] = filled, f
        out[name] = z[:H, :W]
        out[name + "_median"] = np.median(f)
    return out


def first_seed(make, check=lambda d: True):
    for seed in range(1000):
        try:
            d = make(np.random.default_rng(seed))
            if check(d):
                return seed, d
        except MarginError:
            continue
    raise RuntimeError("no seed found")


def store(z, tag, res, rows=None, cols=None):
    for k, v in res.items():
        if tag.endswith("raw") and not k.startswith(("raw_", "n", "margin")):
            continue  # the raw runs are there for the box statistics only
        v = np.asarray(v)
        if k in ("bkg", "rms") and rows is not None:
            v = v[np.ix_(rows, cols)]
        z[f"{tag}_{k}"] = v


def main():
    z = {}

    # case 1: spline parity, 49x56 float64, box (7, 8) -> 7x7 mesh, non-square box
    def make1(rng):
        yy, xx = np.mgrid[:49, :56]
        d = 80.0 + 0.21 * yy - 0.13 * xx + 0.004 * yy * xx + rng.normal(0.0, 2.0, (49, 56))
        for _ in range(4):  # three bright pixels of very different height in one box
            y0, x0 = 7 * rng.integers(0, 7), 8 * rng.integers(0, 7)
            for amp in (4000.0, 300.0, 25.0):
                d[y0 + rng.integers(0, 7), x0 + rng.integers(0, 8)] += amp
        return d

    def full(d, box, filt, **kw):
        """(raw statistics of every box, the case's own result)"""
        return (reference(d, box, (1, 1), exclude_percentile=100.0, **{k: v for k, v in kw.items()
                                                                       if k != "exclude_percentile"}),
                reference(d, box, filt, **kw))

    seed, d1 = first_seed(make1, lambda d: full(d, (7, 8), (3, 3))[0]["niter"].max() >= 3)
    raw, res = full(d1, (7, 8), (3, 3))
    z["c1_data"], z["c1_seed"] = d1, seed
    store(z, "c1raw", raw)
    store(z, "c1", res)

    # case 2: the application's call on the 375x375 float32 golden tile, box 60,
    # filter 3: (a) default exclude_percentile (the 75 %-padding edge row and
    # column are excluded and filled), (b) exclude_percentile=100.  The maps are
    # stored at every 4th row / column plus the last (file size).
    with np.load(os.path.join(OUT, "app_subdiv_inputs.npz")) as f:
        tile = f["img"]
    assert tile.shape == (375, 375) and tile.dtype.itemsize == 4
    idx = np.unique(np.r_[np.arange(0, 375, 4), 374])
    z["c2_idx"] = idx
    raw, res = full(tile, (60, 60), (3, 3))
    assert res["excl"][-1].all() and res["excl"][:, -1].all() and res["excl"].sum() == 13
    assert raw["niter"].max() == 10 and res["niter"].max() == 10  # the cap is reached
    for r_ in (res, reference(tile, (60, 60), (3, 3), exclude_percentile=100.0)):
        lo, hi = r_["bkg_unclipped_range"]  # the clamp is live in both variants
        assert lo < r_["bkg_mesh"].min() or hi > r_["bkg_mesh"].max()
    store(z, "c2raw", raw, idx, idx)
    store(z, "c2a", res, idx, idx)
    resb = reference(tile, (60, 60), (3, 3), exclude_percentile=100.0)
    assert not resb["excl"].any()
    store(z, "c2b", resb, idx, idx)

    # case 3: 21x21, box 7 -> 3x3 mesh: a constant box (0, 0), a box with 5 NaNs
    # (0, 2), the centre box entirely masked (filled from its 8 neighbours).
    # exclude_percentile=20: 5 of 49 invalid pixels (10.2 %) keep a box.
    nan_px = [(1, 15), (2, 18), (3, 16), (5, 20), (6, 14)]

    def make3(rng):
        yy, xx = np.mgrid[:21, :21]
        d = 50.0 + 0.3 * yy + 0.2 * xx + rng.normal(0.0, 1.5, (21, 21))
        d[:7, :7] = 42.5
        d[9, 3] += 90.0
        d[16, 17] += 60.0
        return d

    mask3 = np.zeros((21, 21), bool)
    mask3[7:14, 7:14] = True
    nanmask = np.zeros((21, 21), bool)
    for p in nan_px:
        nanmask[p] = True

    def with_nan(d):
        d = d.copy()
        d[nanmask] = np.nan
        return d

    seed, d3 = first_seed(make3, lambda d: full(with_nan(d), (7, 7), (3, 3), mask=mask3,
                                                exclude_percentile=20.0) is not None)
    raw, res = full(with_nan(d3), (7, 7), (3, 3), mask=mask3, exclude_percentile=20.0)
    assert res["excl"].sum() == 1 and res["excl"][1, 1]
    assert res["nsurv"][0, 0] == 49 and res["raw_med"][0, 0] == 42.5 and res["raw_std"][0, 0] == 0
    assert res["nsurv"][0, 2] <= 44
    z["c3_data"], z["c3_seed"] = d3, seed  # without the NaNs: c3_nanmask says where they go
    z["c3_mask"], z["c3_nanmask"] = mask3, nanmask
    store(z, "c3raw", raw)
    store(z, "c3", res)

    # case 4: 64x128, box 64 -> 1x2 mesh of 4096-pixel boxes (the cap)
    def make4(rng):
        yy, xx = np.mgrid[:64, :128]
        return (120.0 + 0.05 * xx + 0.02 * yy + rng.normal(0.0, 3.0, (64, 128))).astype(np.float32)

    seed, d4 = first_seed(make4, lambda d: full(d, (64, 64), (3, 3)) is not None)
    raw, res = full(d4, (64, 64), (3, 3))
    z["c4_data"], z["c4_seed"] = d4, seed
    store(z, "c4raw", raw)
    store(z, "c4", res)

    # case 5: a batch of three different 21x21 images (float32-representable, so
    # the dtype test can pass the same values as float32 and as float64)
    def make5(rng):
        d = (30.0 + rng.normal(0.0, 2.0, (3, 21, 21)) +
             np.linspace(0, 6, 21)[None, :, None] * np.arange(1, 4)[:, None, None])
        d[0, 4, 4] += 50
        d[2, 18, 2] += 80
        return d.astype(np.float32)

    seed, d5 = first_seed(make5, lambda d: all(full(x, (7, 7), (3, 3)) is not None for x in d))
    z["c5_data"], z["c5_seed"] = d5, seed
    for b in range(3):
        store(z, f"c5i{b}", reference(d5[b], (7, 7), (3, 3)))

    np.savez_compressed(os.path.join(OUT, "bkg2d_cases.npz"), **z)
    print("bkg2d_cases.npz:", os.path.getsize(os.path.join(OUT, "bkg2d_cases.npz")), "bytes;",
          "margins:", {k: float(v) for k, v in z.items() if k.endswith("_margin")})


if __name__ == "__main__":
    main()
