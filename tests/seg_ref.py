"""Plain-numpy restatement of DESIGN §3.8 steps 1-4 (source detection and the
segment catalogue), for the tests that must run where astropy and scipy are
absent: the oversampled Gaussian kernel, the zero-filled padded-sum
convolution, a union-find labeller with the raster-order relabel, and the
per-segment columns.  tests/golden/seg_cases.npz
(tests/golden/make_golden_seg.py) pins it to astropy and scipy."""
import numpy as np

from conftest import golden

FWHM_TO_SIGMA = 1.0 / (2.0 * np.sqrt(2.0 * np.log(2.0)))


def cases():
    return golden("seg_cases.npz")


def make_kernel(fwhm, size, oversample=10):
    """Gaussian of the given FWHM averaged over oversample x oversample
    sub-pixels of each of size x size pixels, normalised to sum 1."""
    sigma = fwhm * FWHM_TO_SIGMA
    f = int(oversample)
    lo, hi = -(size // 2), size // 2 + 1
    x = np.linspace(lo - 0.5 * (1 - 1 / f), hi - 0.5 * (1 + 1 / f), num=int((hi - lo) * f))
    xg, yg = np.meshgrid(x, x)
    # astropy's Gaussian2D.evaluate at theta = 0, operation for operation
    a = 0.5 * (1.0 / sigma ** 2 + 0.0 / sigma ** 2)
    v = 1.0 / (2 * np.pi * sigma * sigma) * np.exp(-((a * xg ** 2) + (0.0 * xg * yg) + (a * yg ** 2)))
    v = v.reshape(size, f, size, f).mean(axis=3).mean(axis=1)
    return v / v.sum()


def convolve(data, kernel):
    """out = (sum_i sum_j P[y+i, x+j] * K[kh-1-i, kw-1-j]) / K.sum(), P the
    zero-padded float64 input, i outer, j inner, every product rounded."""
    d = np.asarray(data).astype(np.float64)
    k = np.asarray(kernel, dtype=np.float64)
    kh, kw = k.shape
    H, W = d.shape
    P = np.zeros((H + kh - 1, W + kw - 1))
    P[kh // 2:kh // 2 + H, kw // 2:kw // 2 + W] = d
    acc = np.zeros((H, W))
    for i in range(kh):
        for j in range(kw):
            acc = acc + P[i:i + H, j:j + W] * k[kh - 1 - i, kw - 1 - j]
    return acc / k.sum()


def label(det, connectivity=8):
    """Components of the boolean image, numbered by their first pixel in
    raster order (what scipy.ndimage.label gives).  Returns (labels, n)."""
    det = np.asarray(det, dtype=bool)
    H, W = det.shape
    parent = np.arange(H * W)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    nb = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for y, x in zip(*np.nonzero(det)):
        p = y * W + x
        for dy, dx in nb:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and det[yy, xx]:
                a, b = find(p), find(yy * W + xx)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    out = np.zeros(H * W, dtype=np.int32)
    n = 0
    number = {}
    for p in np.flatnonzero(det.ravel()):
        r = find(p)  # the smallest index of the component: met first
        if r not in number:
            n += 1
            number[r] = n
        out[p] = number[r]
    return out.reshape(H, W), n


def detect(data, threshold, npixels, connectivity=8, mask=None):
    """photutils' detect_sources: (int32 label image, n); n may be 0."""
    d = np.asarray(data, dtype=np.float64)
    t = np.broadcast_to(np.asarray(threshold, dtype=np.float64), d.shape)
    with np.errstate(invalid="ignore"):
        det = (d > t) & np.isfinite(d) & np.isfinite(t)
    if mask is not None:
        det &= ~np.asarray(mask, dtype=bool)
    lab, n = label(det, connectivity)
    areas = np.bincount(lab.ravel(), minlength=n + 1)
    keep = areas >= npixels
    keep[0] = False
    new = np.zeros(n + 1, dtype=np.int32)
    new[keep] = np.arange(1, keep.sum() + 1)
    return new[lab], int(keep.sum())


def catalog(data, labels, conv=None):
    """The columns of §3.8 step 4 as a dict of arrays over labels 1..n."""
    d = np.asarray(data, dtype=np.float64)
    c = d if conv is None else np.asarray(conv, dtype=np.float64)
    n = int(labels.max())
    names = ("area", "bbox_xmin", "bbox_xmax", "bbox_ymin", "bbox_ymax", "segment_flux",
             "min_value", "max_value", "xcentroid", "ycentroid", "covar_sigx2", "covar_sigxy",
             "covar_sigy2", "abs_flux")
    out = {k: np.zeros(n, dtype=np.int32 if k.startswith(("area", "bbox")) else np.float64)
           for k in names}
    for l in range(1, n + 1):
        yy, xx = np.nonzero(labels == l)
        v, w = d[yy, xx], c[yy, xx]
        sw = w.sum()
        xc, yc = (w * xx).sum() / sw, (w * yy).sum() / sw
        row = (len(yy), xx.min(), xx.max(), yy.min(), yy.max(), v.sum(), v.min(), v.max(), xc, yc,
               (w * (xx - xc) ** 2).sum() / sw, (w * (xx - xc) * (yy - yc)).sum() / sw,
               (w * (yy - yc) ** 2).sum() / sw, np.abs(v).sum())
        for k, val in zip(names, row):
            out[k][l - 1] = val
    return out


def column_bars(cat, shape):
    """The derived bars of the catalogue columns (two summation orders of
    `area` terms): flux 2*area*2^-53*sum|v|; centroid 8*area*2^-53*max(H, W)
    pixels; covariance the centroid bar times max(H, W)."""
    area = cat["area"].astype(np.float64)
    m = float(max(shape))
    u = 2.0 ** -53
    return dict(flux=2 * area * u * cat["abs_flux"], centroid=8 * area * u * m,
                covar=8 * area * u * m * m)


def source_info(data, bkg, rms, n_pixels=5, sigma_threshold=1.5, kernel=None):
    """utils.source_info after its Background2D: (labels, n, sub, conv, thr)."""
    sub = np.asarray(data).astype(np.float64) - bkg
    thr = sigma_threshold * rms
    conv = convolve(sub, make_kernel(1.2, 3) if kernel is None else kernel)
    lab, n = detect(conv, thr, n_pixels)
    return lab, n, sub, conv, thr
