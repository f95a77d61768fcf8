"""Generate tests/golden/seg_cases.npz: inputs and expected outputs of the
device source detection (beta-sgp_amd/segmentation.py).

photutils is not available, so the expected values come from the parts its
``detect_sources`` / ``SourceCatalog`` are built from: the kernel from astropy's
``Gaussian2DKernel`` (astropy 4.3.1), the convolution from
``astropy.convolution.convolve``, the labelling from ``scipy.ndimage.label`` and
the columns from ``scipy.ndimage.find_objects`` / ``sum`` / ``minimum`` /
``maximum`` / ``center_of_mass`` and numpy.  The background maps are
``make_golden_bkg.reference``.  Run from the repository root with the
interpreter make_golden_bkg.py uses (python 3.9):

    PYTHONDONTWRITEBYTECODE=1 python3.9 tests/golden/make_golden_seg.py

The generator asserts for every case that no pixel has
|conv - thr| / max(|conv|, |thr|) below MARGIN, so that a 1e-14 difference in
the rms map cannot move a pixel across the threshold.  The synthetic cases
take the first seed that satisfies it (and the background's own margin).
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import make_golden_bkg as gb  # noqa: E402  (also restores the numpy aliases astropy 4.3.1 needs)
from astropy.convolution import Gaussian2DKernel, convolve  # noqa: E402
from astropy.stats import gaussian_fwhm_to_sigma  # noqa: E402
from scipy import ndimage  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-9
KERNELS = ((1.2, 3), (2.0, 5), (3.0, 7))


def make_kernel(fwhm, size):
    """What photutils' make_2dgaussian_kernel(fwhm, size) builds."""
    k = Gaussian2DKernel(fwhm * gaussian_fwhm_to_sigma, x_size=size, y_size=size,
                         mode="oversample", factor=10)
    k.normalize(mode="integral")
    return k


def detect(conv, thr, npixels):
    det = conv > thr
    lab, n = ndimage.label(det, structure=np.ones((3, 3), int))
    areas = ndimage.sum(det, lab, np.arange(1, n + 1)).astype(int) if n else np.zeros(0, int)
    keep = areas >= npixels
    new = np.zeros(n + 1, dtype=np.int32)
    new[1:][keep] = np.arange(1, keep.sum() + 1)
    return new[lab], int(n), areas


def columns(sub, conv, lab):
    n = int(lab.max())
    idx = np.arange(1, n + 1)
    com = np.array(ndimage.center_of_mass(conv, lab, idx)).reshape(n, 2)
    out = dict(area=ndimage.sum(np.ones_like(sub), lab, idx).astype(np.int32),
               segment_flux=ndimage.sum(sub, lab, idx), abs_flux=ndimage.sum(np.abs(sub), lab, idx),
               min_value=ndimage.minimum(sub, lab, idx), max_value=ndimage.maximum(sub, lab, idx),
               xcentroid=com[:, 1], ycentroid=com[:, 0])
    box = np.zeros((n, 4), dtype=np.int32)
    cov = np.zeros((n, 3))
    for l, sl in enumerate(ndimage.find_objects(lab), start=1):
        box[l - 1] = sl[1].start, sl[1].stop - 1, sl[0].start, sl[0].stop - 1
        w = np.where(lab[sl] == l, conv[sl], 0.0)
        yy, xx = np.mgrid[sl]
        dx, dy = xx - com[l - 1, 1], yy - com[l - 1, 0]
        cov[l - 1] = (w * dx * dx).sum(), (w * dx * dy).sum(), (w * dy * dy).sum()
        cov[l - 1] /= w.sum()
    out.update(bbox_xmin=box[:, 0], bbox_xmax=box[:, 1], bbox_ymin=box[:, 2], bbox_ymax=box[:, 3],
               covar_sigx2=cov[:, 0], covar_sigxy=cov[:, 1], covar_sigy2=cov[:, 2])
    return out


def case(data, box, npix_list, sigma_threshold=1.5):
    res = gb.reference(data, box, (3, 3))
    sub = np.asarray(data).astype(np.float64) - res["bkg"]
    thr = sigma_threshold * res["rms"]
    conv = convolve(sub, make_kernel(1.2, 3), normalize_kernel=True)
    margin = float(np.min(np.abs(conv - thr) / np.maximum(np.abs(conv), np.abs(thr))))
    if margin < MARGIN:
        raise gb.MarginError(f"a pixel lies within {margin:.2e} of the threshold")
    out = dict(bkg=res["bkg"], rms=res["rms"], conv=conv, margin=margin)
    for npix in npix_list:
        lab, nraw, areas = detect(conv, thr, npix)
        out[f"lab{npix}"] = lab.astype(np.int16)
        out["nraw"], out["largest"] = nraw, int(areas.max())
        for k, v in columns(sub, conv, lab).items():
            out[f"n{npix}_{k}"] = v
    return out


def star_field(shape, nblob):
    def make(rng):
        H, W = shape
        yy, xx = np.mgrid[:H, :W]
        d = 100.0 + rng.normal(0.0, 2.0, shape)
        for _ in range(nblob):
            y0, x0, amp = rng.uniform(2, H - 3), rng.uniform(2, W - 3), rng.uniform(8.0, 60.0)
            d += amp * np.exp(-((yy - y0) ** 2 + (xx - x0) ** 2) / (2 * 1.3 ** 2))
        return d.astype(np.float32)
    return make


def main():
    z = {}
    for fwhm, size in KERNELS:
        z[f"kernel_{fwhm}_{size}"] = make_kernel(fwhm, size).array
    z["kernel_list"] = np.array(KERNELS, dtype=np.float64)

    with np.load(os.path.join(OUT, "app_subdiv_inputs.npz")) as f:
        tile = f["img"]
    idx = np.unique(np.r_[np.arange(0, 375, 4), 374])
    z["app_idx"] = idx
    res = case(tile, (60, 60), (5, 1))
    assert res["nraw"] == res["lab1"].max() and res["lab5"].max() < res["lab1"].max()
    for k, v in res.items():
        z[f"app_{k}"] = v[np.ix_(idx, idx)] if k in ("bkg", "rms", "conv") else v
    # the raw tile convolved as it is (its background-subtracted map is not stored in full):
    # an input every test can rebuild exactly, for the bit-equal check on application data
    z["app_rawconv"] = convolve(tile.astype(np.float64), make_kernel(1.2, 3),
                                normalize_kernel=True)[np.ix_(idx, idx)]

    for tag, shape, box, nblob in (("s1", (64, 64), (16, 16), 12), ("s2", (33, 70), (11, 14), 8)):
        def ok(d):
            r = case(d, box, (5,))
            return 0 < r["lab5"].max() < r["nraw"]  # some components are removed
        seed, d = gb.first_seed(star_field(shape, nblob), ok)
        z[f"{tag}_data"], z[f"{tag}_seed"], z[f"{tag}_box"] = d, seed, np.array(box)
        for k, v in case(d, box, (5, 1)).items():
            z[f"{tag}_{k}"] = v

    path = os.path.join(OUT, "seg_cases.npz")
    np.savez_compressed(path, **z)
    print("seg_cases.npz:", os.path.getsize(path), "bytes;",
          {k: (float(v) if k.endswith("margin") else int(v)) for k, v in z.items()
           if k.endswith(("_margin", "_nraw", "_largest"))},
          {t: (int(z[f"{t}_lab5"].max()), int(z[f"{t}_lab1"].max())) for t in ("app", "s1", "s2")})


if __name__ == "__main__":
    main()
