"""astropy's convolve for PSF-sized kernels, without a device:
the numpy restatement tests/conv_ref.py against astropy's recorded outputs
(tests/golden/ref_linear_conv.npz, made by convolve_fft, which computes the
same convolution) and against seg_ref.convolve, the NaN rule on hand-made
cases, the argument checks of convolution.convolve and the validation of
bsgp_convolve2d_ex."""
import ctypes
import inspect

import numpy as np
import pytest

import conv_ref
import seg_ref
from conftest import golden

ODD_CASES = (0, 2, 3)  # the fixture's odd kernels: 9x7 on 40x48, 25x25 on 64x64, 31x31 on 31x31


@pytest.fixture(scope="module")
def lin():
    return golden("ref_linear_conv.npz")


@pytest.mark.parametrize("i", ODD_CASES)
def test_restatement_matches_astropy(lin, i):
    x, k = lin[f"x{i}"], lin[f"k{i}"]
    for kern, want in ((k, lin[f"A{i}"]), (k.conj().T, lin[f"AT{i}"])):
        got = conv_ref.convolve(x, kern)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(f"case {i} {kern.shape}: {err:.2e} of the maximum")
        assert err < 1e-12
        assert np.array_equal(got, seg_ref.convolve(x, kern))
    # a correlation (unflipped kernel) is another function
    corr = conv_ref.convolve(x, k[::-1, ::-1])
    assert np.max(np.abs(corr - lin[f"A{i}"])) / np.max(np.abs(lin[f"A{i}"])) > 1e-3


def test_restatement_options_on_finite_input():
    rng = np.random.default_rng(1)
    d, k = rng.normal(size=(12, 17)), rng.normal(size=(5, 3))
    base, st = conv_ref.convolve(d, k, return_status=True)
    assert st == 0 and np.array_equal(base, seg_ref.convolve(d, k))
    raw = conv_ref.convolve(d, k, normalize_kernel=False)
    assert np.array_equal(raw / k.sum(), base)
    for kw in (dict(nan_treatment="fill"), dict(preserve_nan=True), dict(mask=np.zeros(d.shape, bool))):
        assert np.array_equal(conv_ref.convolve(d, k, **kw), base)
    # a fill value is a constant border: a constant image stays constant under a positive kernel
    kp = np.abs(k)
    c = conv_ref.convolve(np.full((9, 9), 2.5), kp, fill_value=2.5)
    assert np.max(np.abs(c - 2.5)) <= 2 * np.spacing(2.5) * kp.size
    assert not np.array_equal(conv_ref.convolve(d, k, fill_value=2.5), base)


def test_nan_rule_on_hand_made_cases():
    rng = np.random.default_rng(2)
    k = seg_ref.make_kernel(2.0, 5)
    # a constant image with scattered NaNs comes back constant and NaN-free
    # (a power of two: its products with the kernel are exact, so top = 4 * bot to the bit)
    d = np.full((20, 23), 4.0)
    d[rng.integers(0, 20, 12), rng.integers(0, 23, 12)] = np.nan
    got, st = conv_ref.convolve(d, k, fill_value=4.0, return_status=True)
    assert st == conv_ref.HAD_NAN and not np.isnan(got).any()
    assert np.max(np.abs(got - 4.0)) <= 2 * np.spacing(4.0)
    # preserve_nan puts them back, and that alone is not "NaN left"
    got, st = conv_ref.convolve(d, k, fill_value=4.0, preserve_nan=True, return_status=True)
    assert st == conv_ref.HAD_NAN and np.array_equal(np.isnan(got), np.isnan(d))
    # a mask is a NaN
    m = np.isnan(d)
    d2 = np.where(m, 99.0, d)
    assert np.array_equal(conv_ref.convolve(d2, k, fill_value=4.0, mask=m),
                          conv_ref.convolve(d, k, fill_value=4.0))
    # normalize_kernel=False: the interpolated value times the kernel's sum
    k3 = 3.0 * k
    a = conv_ref.convolve(d, k3, fill_value=4.0)
    b = conv_ref.convolve(d, k3, fill_value=4.0, normalize_kernel=False)
    assert np.array_equal(b, a * k3.sum())
    # 'fill': NaNs become the fill value, the sum is the plain one
    f, st = conv_ref.convolve(d, k, nan_treatment="fill", fill_value=1.0, return_status=True)
    assert st == conv_ref.HAD_NAN
    assert np.array_equal(f, seg_ref_fill(np.where(np.isnan(d), 1.0, d), k, 1.0))
    # a NaN block larger than the kernel leaves NaNs and the status bit
    e = rng.normal(size=(20, 23))
    e[4:13, 5:15] = np.nan
    got, st = conv_ref.convolve(e, k, return_status=True)
    assert st == conv_ref.HAD_NAN | conv_ref.NAN_LEFT
    want = np.zeros(e.shape, bool)
    want[6:11, 7:13] = True  # windows that lie inside the block: bot == 0, the centre is NaN
    assert np.array_equal(np.isnan(got), want)
    # a +inf / -inf pair is no NaN in the input: the flag stays clear, the plain rule applies
    g = rng.normal(size=(20, 23))
    g[3, 3], g[3, 5] = np.inf, -np.inf
    got, st = conv_ref.convolve(g, k, return_status=True)
    assert not (st & conv_ref.HAD_NAN) and (st & conv_ref.NAN_LEFT)
    with np.errstate(invalid="ignore"):
        plain = seg_ref.convolve(g, k)
    assert np.array_equal(got, plain, equal_nan=True) and np.isnan(got[3, 4])


def seg_ref_fill(d, k, fill):
    """seg_ref.convolve with a constant border: the image embedded in a frame of the
    fill value wide enough that the zero fill beyond it touches no kept pixel."""
    kh, kw = k.shape
    big = np.full((d.shape[0] + 2 * kh, d.shape[1] + 2 * kw), float(fill))
    big[kh:-kh, kw:-kw] = d
    return seg_ref.convolve(big, k)[kh:-kh, kw:-kw]


def test_fill_value_equals_an_embedded_frame():
    rng = np.random.default_rng(3)
    d, k = rng.normal(size=(11, 9)), rng.normal(size=(7, 5))
    assert np.array_equal(conv_ref.convolve(d, k, fill_value=2.5), seg_ref_fill(d, k, 2.5))


def test_gaussian_kernel_pairs():
    import convolution as cv
    import segmentation as sg
    for n in (3, 7, 31):
        assert np.array_equal(cv.make_2dgaussian_kernel(1.2, n), sg.make_2dgaussian_kernel(1.2, n))
        assert np.array_equal(cv.make_2dgaussian_kernel(1.2, (n, n)), sg.make_2dgaussian_kernel(1.2, n))
    k = cv.make_2dgaussian_kernel(1.2, (31, 25))
    assert k.shape == (31, 25) and abs(k.sum() - 1) < 1e-15
    sq = sg.make_2dgaussian_kernel(1.2, 31)  # a separable Gaussian: the centre columns, renormalised
    np.testing.assert_allclose(k, sq[:, 3:28] / sq[:, 3:28].sum(), rtol=1e-12)
    for bad in (4, (31, 24), (3, 3, 3), 0, 2.5):
        with pytest.raises(ValueError, match="size"):
            cv.make_2dgaussian_kernel(1.2, bad)


def test_argument_errors_need_no_device():
    import convolution as cv
    img = np.ones((21, 21))
    k = np.ones((3, 3))
    for bad in ("extend", "wrap", None):
        with pytest.raises(ValueError, match="boundary.*out of scope"):
            cv.convolve(img, k, boundary=bad)
    with pytest.raises(ValueError, match="nan_treatment"):
        cv.convolve(img, k, nan_treatment="ignore")
    for bad in (np.ones((2, 2)), np.ones((3, 4)), np.ones((65, 65)), np.ones((3, 65)), np.ones(3),
                np.ones((2, 3, 3)), np.full((3, 3), np.nan), np.full((3, 3), np.inf)):
        with pytest.raises(ValueError, match="kernel"):
            cv.convolve(img, bad)
    with pytest.raises(ValueError, match="kernel"):  # per-image kernels: one per image
        cv.convolve(np.ones((2, 21, 21)), np.ones((3, 3, 3)))
    with pytest.raises(ValueError, match="mask shape"):
        cv.convolve(img, k, mask=np.zeros((21, 20), bool))
    for bad in (np.nan, np.inf, "x"):
        with pytest.raises(ValueError, match="fill_value"):
            cv.convolve(img, k, fill_value=bad)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        cv.convolve(np.ones(21), k)
    s = inspect.signature(cv.convolve)
    assert [(n, p.default) for n, p in s.parameters.items()][2:] == [
        ("boundary", "fill"), ("fill_value", 0.0), ("nan_treatment", "interpolate"),
        ("normalize_kernel", True), ("mask", None), ("preserve_nan", False),
        ("normalization_zero_tol", 1e-8), ("device_out", False)]
    assert list(inspect.signature(cv.scale_psf).parameters)[:3] == ["psf", "gaussian_fwhm", "size"]
    assert inspect.signature(cv.scale_psf).parameters["gaussian_fwhm"].default == 1.2
    assert list(inspect.signature(cv.degrade).parameters)[:2] == ["image", "psf"]


def test_normalisation_test_is_astropys():
    import convolution as cv
    shape = (21, 21)
    one = np.zeros((3, 3))

    def kern(s):
        k = one.copy()
        k[1, 1] = s
        return k

    zero = np.array([[0, 1, 0], [0, -1, 0], [0, 0, 0.0]])
    for k, tol in ((zero, 1e-8), (kern(0.005), 1e-8), (kern(1e-5), 1e-4)):
        with pytest.raises(ValueError, match="can't be normalized"):
            cv.check_convolve_args(shape, k, normalization_zero_tol=tol)
    # not asked to normalise: no test; a sum of 0.02 passes it
    for k in (zero, kern(0.005)):
        assert cv.check_convolve_args(shape, k, normalize_kernel=False)[1][0] == k.sum()
    kk, sums = cv.check_convolve_args(shape, kern(0.02))
    assert sums.shape == (1,) and sums[0] == 0.02 and kk.flags.c_contiguous
    # per-image kernels: numpy's sum of each, and each is tested
    rng = np.random.default_rng(4)
    ks = rng.random((3, 31, 31))
    kk, sums = cv.check_convolve_args((3,) + shape, ks)
    assert np.array_equal(sums, [ks[0].sum(), ks[1].sum(), ks[2].sum()])
    ks[1] *= 1e-6
    with pytest.raises(ValueError, match="can't be normalized"):
        cv.check_convolve_args((3,) + shape, ks)


def test_no_cpu_fallback():
    import _bsgp
    import convolution as cv
    if _bsgp.torch is not None and _bsgp.torch.cuda.is_available():
        return  # tests/test_gpu_convolution.py runs it
    img, psf = np.ones((21, 21)), np.ones((5, 5))
    for call in (lambda: cv.convolve(img, psf), lambda: cv.degrade(img, psf),
                 lambda: cv.scale_psf(psf)):
        with pytest.raises(_bsgp.BsgpError):
            call()


def test_c_abi_argument_errors():
    """bsgp_convolve2d_ex validates on the host before any device call."""
    import _bsgp
    L = _bsgp.lib()
    assert "bsgp_convolve2d_ex" in _bsgp.EXPORTED and hasattr(L, "bsgp_convolve2d_ex")
    assert L.bsgp_abi_version() == 3
    buf = np.zeros((64, 64))
    p = ctypes.c_void_p(buf.ctypes.data)  # never dereferenced: every call below fails validation

    def conv(data=p, dtype=1, B=1, H=64, W=64, kernel=p, kh=31, kw=31, stride=0, ksum=p, flags=2,
             fill=0.0, out=p, status=p):
        rc = L.bsgp_convolve2d_ex(data, dtype, B, H, W, kernel, kh, kw, stride, ksum, None, flags,
                                  fill, out, status, None)
        return rc, L.bsgp_last_error().decode()

    for kw, word in ((dict(data=None), "data"), (dict(kernel=None), "kernel"),
                     (dict(ksum=None), "kernel_sum"), (dict(out=None), "out"),
                     (dict(status=None), "status_out"), (dict(dtype=2), "dtype"),
                     (dict(B=0), "B"), (dict(H=0), "H"), (dict(kh=0), "kernel size"),
                     (dict(stride=5), "kernel_stride"), (dict(flags=8), "flags"),
                     (dict(fill=np.nan), "fill_value"), (dict(fill=np.inf), "fill_value")):
        rc, msg = conv(**kw)
        assert rc == _bsgp.BSGP_ERR_ARG and word in msg, (kw, rc, msg)
    for kw in (dict(kh=4), dict(kw=2), dict(kh=65), dict(kw=65)):
        rc, msg = conv(**kw)
        assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and "63 x 63" in msg, (kw, rc, msg)
    rc, msg = conv(H=65536, W=32768)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and "2^31" in msg, (rc, msg)
    rc, msg = conv(B=65536)
    assert rc == _bsgp.BSGP_ERR_UNSUPPORTED and "65535" in msg, (rc, msg)
    assert (_bsgp.BSGP_CONV_MAX_KERNEL, _bsgp.BSGP_CONV_HAD_NAN, _bsgp.BSGP_CONV_NAN_LEFT) == (63, 1, 2)
