"""numpy restatement of the background estimator's spline stage (DESIGN §3.7
step 7), shared by tests/test_background.py and tests/test_gpu_background.py:
scipy.ndimage's cubic prefilter (mode='reflect') and the evaluation of a
coefficient mesh at the zoom's sample points."""
import numpy as np

from conftest import golden

Z = np.sqrt(3.0) - 2.0


def cases():
    return golden("bkg2d_cases.npz")


def prefilter_line(c):
    """scipy.ndimage.spline_filter1d(c, 3, mode='reflect'): gain 6, pole
    sqrt(3) - 2; the causal start accumulates into c[0] in place (so its last
    term reads the partial sum), the anticausal start is c[n-1] * z / (z - 1)."""
    c = np.array(c, dtype=np.float64)
    n = len(c)
    if n <= 1:
        return c
    c *= 6.0
    zn = 1.0
    for _ in range(n):
        zn *= Z
    c0 = c[0]
    c[0] = c0 + zn * c[n - 1]
    zi = Z
    for i in range(1, n):
        c[0] += zi * (c[i] + zn * c[n - 1 - i])
        zi *= Z
    c[0] *= Z / (1.0 - zn * zn)
    c[0] += c0
    for i in range(1, n):
        c[i] += Z * c[i - 1]
    c[n - 1] *= Z / (Z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = Z * (c[i + 1] - c[i])
    return c


def coefficients(mesh):
    """Spline coefficients of a mesh: the prefilter along y, then along x."""
    c = np.array(mesh, dtype=np.float64)
    for x in range(c.shape[1]):
        c[:, x] = prefilter_line(c[:, x])
    for y in range(c.shape[0]):
        c[y] = prefilter_line(c[y])
    return c


def taps(n_out, box, n):
    """Indices [n_out, 4] (half-sample symmetric) and weights [n_out, 4] of the
    cubic B-spline at mesh coordinate (p + 0.5) / box - 0.5; an axis of one
    cell is constant."""
    p = np.arange(n_out, dtype=np.float64)
    if n == 1:
        return np.zeros((n_out, 4), int), np.tile([1.0, 0.0, 0.0, 0.0], (n_out, 1))
    cc = (p + 0.5) / box - 0.5
    fl = np.floor(cc)
    t = cc - fl
    z = 1.0 - t
    w = np.empty((n_out, 4))
    w[:, 1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 0] = z * z * z / 6.0
    w[:, 3] = 1.0 - w[:, 0] - w[:, 1] - w[:, 2]
    idx = fl.astype(int)[:, None] - 1 + np.arange(4)[None, :]
    idx = np.where(idx < 0, -idx - 1, idx)
    idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    return idx, w


def zoom(mesh, box, shape, clip=True):
    """The map [H, W] of a filtered mesh: coefficients, evaluation (rows folded
    first, then columns), clamp to the mesh's range."""
    coef = coefficients(mesh)
    ny, nx = coef.shape
    iy, wy = taps(shape[0], box[0], ny)
    ix, wx = taps(shape[1], box[1], nx)
    line = sum(wy[:, a, None] * coef[iy[:, a], :] for a in range(4))  # [H, nx]
    out = sum(wx[None, :, b] * line[:, ix[:, b]] for b in range(4))
    return np.clip(out, np.min(mesh), np.max(mesh)) if clip else out
