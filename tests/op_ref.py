"""An exact reference of the operators A / AT, without an FFT, and the table of
shapes the operator sweep runs (tests/test_op_ref.py on the host,
tests/test_gpu_opsweep.py on the device).

circ_ref and lin_ref evaluate the convolution sums tap by tap.  Where
np.longdouble is an extended type (eps < 1e-18: x87's 64-bit significand,
eps = 2**-63; IEEE binary128) the sums run in it: every product k * x of two
float64 values rounds once (relative 2**-64), the running sum is error-free
(TwoSum: the rounding error of every addition is kept in a second word), the
two words are added once at the end and lin_ref divides once by the kernel's
sum.  So every pixel is within 3 * 2**-64 * sum|k * x| < 1.7e-19 * sum|terms|
of the true value (2 * 2**-64 for circ_ref), plus terms of second order: more
than 1000 times below float64's eps = 2.2e-16, whatever the number of taps.
Where np.longdouble is float64 (eps >= 1e-18) the same sums run in
double-double: TwoProduct (Veltkamp / Dekker) makes the products exact too,
and a pixel is within about 1e-30 * sum|terms|.  Both forms return an Exact
(two words hi + lo; lo is zero in the extended form), and `errors` subtracts a
float64 result from it without rounding the reference to float64.

numpy's own float64 FFT operators (sgp_oracle.make_operators) differ from
this reference by 2-4e-16 in relative L2 and 2-9e-16 of max|ref| in max-norm
(tests/test_op_ref.py asserts <= 4e-15 for every shape of the table).
"""
import ctypes
import math

import numpy as np

LD = np.longdouble
EXTENDED = bool(np.finfo(LD).eps < 1e-18)

LIN, CIRC = 1, 0  # bsgp.h BSGP_CONV_LINEAR_FILL / BSGP_CONV_CIRCULAR


# ------------------------------------------------------------ exact arithmetic
def _two_sum(a, b):
    """s + e == a + b exactly (Knuth)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a  # 2**27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _prod_err(a, b, p):
    """a * b - p exactly, for float64 a, b and p = fl(a * b) (Dekker)."""
    ah, al = _split(a)
    bh, bl = _split(b)
    return ((ah * bh - p) + ah * bl + al * bh) + al * bl


class Exact:
    """hi + lo, elementwise: the reference's value in more than one float64."""

    def __init__(self, hi, lo):
        self.hi, self.lo = hi, lo

    @property
    def shape(self):
        return self.hi.shape

    def __getitem__(self, i):
        return Exact(self.hi[i], self.lo[i])

    def __array__(self, dtype=None, copy=None):
        v = self.hi + self.lo
        return v if dtype is None else v.astype(dtype)

    def minus(self, out):
        """out - self, in the reference's precision."""
        return (np.asarray(out).astype(self.hi.dtype) - self.hi) - self.lo


class _Acc:
    """sum of k * x over taps: s the rounded running sum, c the sum of the
    additions' (and, in double-double, the products') rounding errors."""

    def __init__(self, shape, extended):
        self.ext = extended
        self.t = LD if extended else np.float64
        self.s = np.zeros(shape, self.t)
        self.c = np.zeros(shape, self.t)
        # work arrays of the in-place TwoSum (a temporary per operation costs
        # more than the arithmetic)
        self.w = [np.empty(shape, self.t) for _ in range(4)]

    def add(self, k, xs, dst):
        k = self.t(k)
        s, c = self.s[dst], self.c[dst]
        p, t, b, u = (w[dst] for w in self.w)
        np.multiply(xs, k, out=p)
        if not self.ext:
            c += _prod_err(k, xs, p)
        np.add(s, p, out=t)  # _two_sum(s, p) -> t, u
        np.subtract(t, s, out=b)
        np.subtract(t, b, out=u)
        np.subtract(s, u, out=u)
        np.subtract(p, b, out=p)
        u += p
        c += u
        s[...] = t

    def result(self):
        return Exact(*_two_sum(self.s, self.c))


def _mode(extended):
    extended = EXTENDED if extended is None else bool(extended)
    if extended and not EXTENDED:
        raise ValueError("np.longdouble is float64 here")
    return extended


def circ_ref(x, psf, transpose=False, extended=None):
    """The circular operator of sgp_oracle.make_operators(psf, shape, True):
    real(ifftn(fftn(fftshift(psf)) * fftn(x))), with the conjugate transfer
    function for `transpose`.  x: [..., H, W] float64, psf: [H, W] float64."""
    ext = _mode(extended)
    x = np.asarray(x, np.float64)
    psf = np.asarray(psf, np.float64)
    H, W = psf.shape
    assert x.shape[-2:] == (H, W)
    acc = _Acc(x.shape, ext)
    sgn = -1 if transpose else 1
    for a, b in np.argwhere(psf != 0):
        sa, sb = (a + H // 2) % H, (b + W // 2) % W
        acc.add(psf[a, b], np.roll(x, (sgn * sa, sgn * sb), (-2, -1)), Ellipsis)
    return acc.result()


def _sum2(k, ext):
    """sum(k) as (hi, lo)."""
    if ext:
        return k.astype(LD).sum(), LD(0)
    hi = math.fsum(k.ravel())
    return np.float64(hi), np.float64(math.fsum(list(k.ravel()) + [-hi]))


def _div(r, sh, sl):
    """Exact r / (sh + sl)."""
    if r.hi.dtype == LD:
        return Exact(np.asarray(r) / sh, np.zeros(r.shape, LD))
    q1 = r.hi / sh
    p = q1 * sh
    rem = ((r.hi - p) - _prod_err(q1, sh, p)) + r.lo - q1 * sl
    return Exact(*_two_sum(q1, rem / sh))


def lin_ref(x, k, transpose=False, extended=None):
    """The zero-filled linear operator of make_operators(k, shape, False)
    (astropy's convolve_fft with normalize_kernel, boundary="fill"): the kernel
    k / k.sum(), or its transpose k.T (not a flip) for `transpose`; tap (u, v)
    shifts the image by (u - kh // 2, v - kw // 2).  x: [..., H, W] float64."""
    ext = _mode(extended)
    x = np.asarray(x, np.float64)
    k = np.asarray(k, np.float64)
    if transpose:
        k = k.T
    kh, kw = k.shape
    H, W = x.shape[-2:]
    acc = _Acc(x.shape, ext)
    for u in range(kh):
        du = u - kh // 2
        i0, i1 = max(0, du), min(H, H + du)
        if i0 >= i1:
            continue
        for v in range(kw):
            dv = v - kw // 2
            j0, j1 = max(0, dv), min(W, W + dv)
            if j0 >= j1 or k[u, v] == 0:
                continue
            acc.add(k[u, v], x[..., i0 - du:i1 - du, j0 - dv:j1 - dv],
                    (Ellipsis, slice(i0, i1), slice(j0, j1)))
    return _div(acc.result(), *_sum2(k, ext))


def op_ref(x, psf, mode, transpose=False):
    return (lin_ref if mode == LIN else circ_ref)(x, psf, transpose)


def errors(out, ref):
    """(relative L2, max|out - ref| / max|ref|) of a float64 result."""
    d = ref.minus(out)
    r = np.asarray(ref)
    l2 = np.sqrt((d * d).sum()) / max(np.sqrt((r * r).sum()), np.finfo(np.float64).tiny)
    mx = np.abs(d).max() / max(np.abs(r).max(), np.finfo(np.float64).tiny)
    return float(l2), float(mx)


def numpy_op(x, psf, mode, transpose=False):
    """numpy's float64 FFT operator (the oracle's) on a batch [B, H, W]."""
    import sgp_oracle
    A, AT = sgp_oracle.make_operators(psf, x.shape[-2:], mode == CIRC)
    f = AT if transpose else A
    return np.stack([f(xi.ravel()).reshape(xi.shape) for xi in x])


# The tolerance of the device operators against this reference, per case and
# per norm: FACTOR times the error of numpy's float64 operator in that case
# and norm (a margin over the reference's error for another radix order,
# direct-DFT prime stages and the ~1 ulp two-level twiddle products), never
# looser than the suite's earlier bar (1e-13 relative L2) or 1e-12 in max-norm.
FACTOR = 8.0
L2_CAP, MAX_CAP = 1e-13, 1e-12


def tolerances(np_l2, np_max, factor=FACTOR):
    return min(factor * np_l2, L2_CAP), min(factor * np_max, MAX_CAP)


# ------------------------------------------------------------ the sweep table
FIELDS = ["H", "W", "P", "Q", "Qh", "sld", "lpad", "nfw", "nfc", "coop", "tw2", "twmix",
          "fp_lds_tw", "fq_lds_tw", "fp_lds_tw2", "fq_lds_tw2", "lds_fft_bytes", "lds_bytes",
          "wg_per_cu", "vec_stride", "spec_off", "slot_stride", "fp_ns", "fq_ns"]


def plan_layout(H, W, kh, kw, mode, storage=0):
    """bsgp_plan_layout's fields by name, with the stage radices of the column
    (fp_radix) and row (fq_radix) transforms.  Needs no GPU."""
    import _bsgp
    L = _bsgp.lib()
    L.bsgp_plan_layout.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_void_p, ctypes.c_int32]
    out = np.zeros(len(FIELDS) + 32, np.int64)
    rc = L.bsgp_plan_layout(H, W, kh, kw, mode, storage, out.ctypes.data, len(out))
    if rc != 0:
        raise _bsgp.BsgpError(rc, L.bsgp_last_error().decode())
    g = dict(zip(FIELDS, map(int, out)))
    g["fp_radix"] = [int(v) for v in out[24:24 + g["fp_ns"]]]
    g["fq_radix"] = [int(v) for v in out[40:40 + g["fq_ns"]]]
    return g


class Case:
    """One row of the sweep: the image, the mode, the kernel's shape (linear)
    and the plan_layout values that make it the case it is listed as."""

    def __init__(self, H, W, mode, kshape=None, **pin):
        self.H, self.W, self.mode = H, W, mode
        self.kshape = tuple(kshape) if kshape else (H, W)
        self.pin = pin

    @property
    def id(self):
        k = "" if self.mode == CIRC else "-k%dx%d" % self.kshape
        return "%dx%d-%s%s" % (self.H, self.W, "circ" if self.mode == CIRC else "lin", k)

    def layout(self):
        return plan_layout(self.H, self.W, self.kshape[0], self.kshape[1], self.mode)

    def seed(self):
        return [self.H, self.W, self.mode, self.kshape[0], self.kshape[1]]

    def psf(self, variant=0):
        """A normalised kernel.  Circular: full-size, at most 40 non-zero taps,
        [0, 0] and [-1, -1] among them.  Linear: dense, except on images above
        128 x 128 with kernels above 100 taps (256 x 256 with 25 x 25), which
        take 40 taps like the circular ones, the corners among them: the
        reference costs a pass over the image per tap."""
        rng = np.random.default_rng(self.seed() + [1, variant])
        kh, kw = self.kshape
        if self.mode == LIN and (kh * kw <= 100 or self.H * self.W <= 128 * 128):
            k = rng.uniform(0.1, 1.0, self.kshape)
            return k / k.sum()
        p = np.zeros(kh * kw)
        idx = rng.choice(p.size, min(38, p.size), replace=False)
        p[idx] = rng.uniform(0.1, 1.0, idx.size)
        p = p.reshape(kh, kw)
        p[0, 0] = 0.7
        p[-1, -1] = 0.4
        if self.mode == LIN:
            p[0, -1] = 0.3
            p[-1, 0] = 0.2
        return p / p.sum()

    def images(self, variant=0):
        """[3, H, W]: uniform(0, 1) with two bright corner pixels; zero but for
        the last row and the last column; all zero."""
        rng = np.random.default_rng(self.seed() + [2, variant])
        x = np.zeros((3, self.H, self.W))
        x[0] = rng.uniform(0, 1, (self.H, self.W))
        x[0, 0, 0] = 50.0
        x[0, -1, -1] = 80.0
        x[1, -1, :] = rng.uniform(0, 1, self.W)
        x[1, :, -1] = rng.uniform(0, 1, self.H)
        return x


def _c(H, W, **pin):
    return Case(H, W, CIRC, None, **pin)


def _l(H, W, kh, kw, **pin):
    return Case(H, W, LIN, (kh, kw), **pin)


# Every row with the plan_layout values it is there for ("tw_lds": whether the
# per-wave twiddle tables are in LDS; the radices are fp's, columns, and fq's,
# rows).  tests/test_op_ref.py::test_sweep_row_lands_in_its_branch holds
# plan_layout to them.
SWEEP = [
    # degenerate lengths: no stage at all, a lone unpaired row, Qh = 1
    _c(1, 1, P=1, Q=1, Qh=1, fp_ns=0, fq_ns=0, coop=0),
    _c(2, 3, fp_radix=[2], fq_radix=[3], Qh=2, coop=0),
    _c(1, 64, P=1, fp_ns=0, Q=64, sld=2, coop=0),
    _c(64, 1, Q=1, Qh=1, fq_ns=0, P=64, coop=0),
    # a single prime stage each way
    _c(7, 11, fp_radix=[7], fq_radix=[11], sld=8),
    # radices 4 2 3 / 4 5, P != Q
    _c(24, 20, fp_radix=[4, 2, 3], fq_radix=[4, 5], coop=0, wg_per_cu=4),
    # prime stages behind other stages; odd H
    _c(49, 77, fp_radix=[7, 7], fq_radix=[7, 11], sld=50),
    _c(62, 93, fp_radix=[2, 31], fq_radix=[3, 31], sld=62),
    # even, non-square kernels (AT is kw x kh); odd / even H and W
    _l(33, 31, 6, 8, P=40, Q=36, sld=34, coop=0, wg_per_cu=4),
    _l(45, 50, 5, 3, P=48, Q=54, sld=46, coop=0),
    # a kernel about the size of the image, and one larger than it (pmin < km)
    _l(40, 36, 31, 31, P=60, Q=54),
    _l(5, 7, 9, 4, P=9, Q=12, sld=6),
    # the compile-time 270- and 256-point transforms (twiddles in LDS)
    _l(256, 256, 25, 25, P=270, Q=270, coop=0, wg_per_cu=4, tw_lds=True),
    _c(256, 256, P=256, Q=256, coop=0, wg_per_cu=4, tw_lds=True),
    # per-wave, four per CU, twiddles from global memory
    _c(300, 288, coop=0, wg_per_cu=4, tw_lds=False),
    _c(288, 300, coop=0, wg_per_cu=4, tw_lds=False),
    # three per CU: P != Q with sld padding; a radix-17 stage
    _l(301, 290, 9, 5, coop=0, wg_per_cu=3, P=320, Q=300, sld=302, tw_lds=True),
    _c(340, 340, coop=0, wg_per_cu=3, fp_radix=[4, 5, 17], tw_lds=True),
    # two per CU (the 400-point transform is the runtime plan in this build)
    _c(360, 300, coop=0, wg_per_cu=2, tw_lds=True),
    _c(400, 400, coop=0, wg_per_cu=2, fp_radix=[4, 4, 5, 5], tw_lds=True),
    # cooperative: four groups; two groups with the long axis on rows / columns
    _c(512, 486, coop=1, nfw=4, nfc=4),
    _c(8, 600, coop=1, nfw=2, nfc=2, P=8, Q=600),
    _c(600, 8, coop=1, nfw=2, nfc=2, P=600, Q=8),
    # cooperative with a radix-41 stage, nfc < nfw, odd H
    _c(1025, 6, coop=1, nfw=2, nfc=1, fp_radix=[5, 5, 41], sld=1026),
    # the two-level table for Q only (no stage tables); for P only, with them
    _c(4, 2048, coop=1, fq_lds_tw2=0, fp_lds_tw2=-1, twmix=-1, tw2=1536),
    _c(2048, 6, coop=1, fp_lds_tw2=0, fq_lds_tw2=-1, twmix=1536, tw2=10752),
    # P = 2025 = 3^4 5^2: a cooperative runtime plan, one workgroup per CU
    _l(2000, 10, 9, 9, coop=1, P=2025, fp_radix=[3, 3, 3, 3, 5, 5], wg_per_cu=1),
    # cooperative, one group
    _c(9, 2500, coop=1, nfw=1, nfc=1),
]
BY_ID = {c.id: c for c in SWEEP}

# the rows whose batch paths, per-image PSFs and short solves are run
BATCH = ["24x20-circ", "33x31-lin-k6x8", "8x600-circ", "2048x6-circ"]
PER_IMAGE = ["33x31-lin-k6x8", "24x20-circ", "8x600-circ"]
SOLVE = ["33x31-lin-k6x8", "45x50-lin-k5x3", "49x77-circ", "300x288-circ", "8x600-circ",
         "600x8-circ", "4x2048-circ"]


def misplaced(case, g=None):
    """The pinned layout values the plan of `case` does not have: {} when the
    row is in its branch."""
    g = case.layout() if g is None else g
    bad = {}
    for k, want in case.pin.items():
        got = (g["fp_lds_tw"] >= 0 and g["fq_lds_tw"] >= 0) if k == "tw_lds" else g[k]
        if got != want:
            bad[k] = (got, want)
    return bad
