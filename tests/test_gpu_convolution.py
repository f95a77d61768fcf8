"""astropy's convolve for PSF-sized kernels on the device
(beta-sgp_amd/convolution.py, bsgp_convolve2d_ex) against the
numpy restatement tests/conv_ref.py, bit for bit: both sum every pixel's taps
in the same order and round every product and sum.  The shapes are the
smallest that reach every branch of the tiled kernel: images smaller than the
halo, off-tile sizes with interior tiles and all four borders, 1 x 63 and
63 x 1 and 63 x 63 kernels, every rows-per-thread build (1, 2, 4, 8)."""
import warnings

import numpy as np
import pytest

import conv_ref
import seg_ref
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv():
    import _bsgp
    _bsgp.require_gpu()
    import convolution
    return convolution


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


SHAPES = [((1, 1), (31, 31)), ((3, 3), (31, 31)), ((1, 300), (31, 31)), ((70, 1), (31, 31)),
          ((31, 31), (31, 31)), ((33, 70), (25, 25)), ((70, 130), (31, 31)), ((40, 48), (9, 7)),
          ((9, 520), (1, 63)), ((520, 9), (63, 1)), ((64, 64), (63, 63)), ((6, 70), (5, 5)),
          ((13, 65), (3, 7))]


@pytest.mark.parametrize("shape,ksz", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_bit_equal_to_the_restatement(cv, shape, ksz):
    rng = np.random.default_rng(11)
    d = rng.normal(10.0, 3.0, shape)
    k = rng.uniform(-0.2, 1.0, ksz)  # negative entries too
    got = cv.convolve(d, k)
    assert got.dtype == np.float64 and got.status == 0
    assert same(got, conv_ref.convolve(d, k)), (shape, ksz)
    assert same(cv.convolve(d, k, fill_value=2.5), conv_ref.convolve(d, k, fill_value=2.5))
    assert same(cv.convolve(d, k, normalize_kernel=False),
                conv_ref.convolve(d, k, normalize_kernel=False))
    d32 = d.astype(np.float32)
    a = cv.convolve(d32, k)
    assert same(a, cv.convolve(d32.astype(np.float64), k)) and same(a, conv_ref.convolve(d32, k))


def test_batch_with_per_image_kernels(cv):
    rng = np.random.default_rng(12)
    d = rng.normal(10.0, 3.0, (3, 37, 71))
    ks = rng.uniform(-0.2, 1.0, (3, 31, 31))
    got = cv.convolve(d, ks)
    want, st = conv_ref.convolve_batch(d, ks)
    assert same(got, want) and np.array_equal(got.status, st)
    for b in range(3):
        assert same(cv.convolve(d[b], ks[b]), got[b])
    assert same(cv.convolve(d, ks), got)  # a second run gives the same bits
    one = cv.convolve(d, ks[1])  # one kernel for all
    assert same(one, conv_ref.convolve_batch(d, ks[1])[0]) and same(one[1], got[1])
    import _bsgp
    t = _bsgp.torch.from_numpy(d).to("cuda")
    out, status = cv.convolve(t, ks, device_out=True)
    assert out.is_cuda and same(out.cpu().numpy(), want) and status.cpu().tolist() == [0, 0, 0]


@pytest.mark.parametrize("n", (3, 5, 7))
def test_equals_the_segmentation_path(cv, n):
    """Where the old path exists (kernels up to 7 x 7) both give the same bits."""
    import segmentation as sg
    rng = np.random.default_rng(13)
    d, k = rng.normal(10.0, 3.0, (40, 257)), rng.uniform(-0.2, 1.0, (n, n))
    assert same(cv.convolve(d, k), sg.convolve(d, k))
    assert same(cv.convolve(d, k), seg_ref.convolve(d, k))


# ------------------------------------------------------------------ NaN rule
def nan_cases():
    rng = np.random.default_rng(14)
    base = rng.normal(10.0, 3.0, (45, 70))
    yy, xx = np.mgrid[:45, :70]
    one = base.copy()
    one[20, 33] = np.nan
    row = base.copy()
    row[0, :] = np.nan
    row[:, 69] = np.nan
    disc = (yy - 22) ** 2 + (xx - 40) ** 2 <= 36
    block = base.copy()
    block[5:30, 10:40] = np.nan
    return dict(one=(one, None), border=(row, None), disc=(base, disc), block=(block, None))


@pytest.mark.parametrize("name", ("one", "border", "disc", "block"))
@pytest.mark.parametrize("opts", (dict(), dict(nan_treatment="fill", fill_value=1.5),
                                  dict(preserve_nan=True), dict(normalize_kernel=False),
                                  dict(nan_treatment="fill", preserve_nan=True)),
                         ids=("interpolate", "fill", "preserve", "unnormalized", "fill-preserve"))
def test_nan_rule(cv, name, opts):
    d, m = nan_cases()[name]
    k = np.random.default_rng(15).uniform(0.0, 1.0, (13, 11))
    want, st = conv_ref.convolve(d, k, mask=m, return_status=True, **opts)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = cv.convolve(d, k, mask=m, **opts)
    assert same(got, want), (name, opts)
    assert got.status == st and (st & conv_ref.HAD_NAN)
    assert bool(st & conv_ref.NAN_LEFT) == any(issubclass(x.category, cv.NaNLeftWarning) for x in w)
    if name == "block" and opts.get("nan_treatment") != "fill":
        # windows inside the block stay NaN; with preserve_nan every one of them is a
        # pixel that was NaN, so none counts as left
        assert np.isnan(got[15:20, 20:30]).all()
        assert bool(st & conv_ref.NAN_LEFT) == (not opts.get("preserve_nan"))
    if name != "block" and not opts.get("preserve_nan"):
        assert st == conv_ref.HAD_NAN and not np.isnan(got).any()
    if opts.get("preserve_nan"):
        was = np.isnan(d) if m is None else m
        assert np.isnan(got[was]).all()


def test_only_the_image_with_a_nan_is_interpolated(cv):
    rng = np.random.default_rng(16)
    d = rng.normal(10.0, 3.0, (3, 33, 70))
    d[1, 10, 12] = np.nan
    d[2, 4, 4], d[2, 4, 9] = np.inf, -np.inf  # no NaN in the input: the flag stays clear
    k = rng.uniform(0.0, 1.0, (25, 25))
    with pytest.warns(cv.NaNLeftWarning):
        got = cv.convolve(d, k)
    want, st = conv_ref.convolve_batch(d, k)
    assert same(got, want) and np.array_equal(got.status, st)
    assert list(got.status) == [0, conv_ref.HAD_NAN, conv_ref.NAN_LEFT]
    with np.errstate(invalid="ignore"):
        assert same(got[0], seg_ref.convolve(d[0], k)) and same(got[2], seg_ref.convolve(d[2], k))
    assert not np.isnan(got[1]).any() and not same(got[1], seg_ref.convolve(d[1], k))


# ------------------------------------------------------------- astropy's bits
@pytest.mark.parametrize("i", (0, 2, 3))
def test_matches_astropy_fixture(cv, i):
    lin = golden("ref_linear_conv.npz")
    x, k = lin[f"x{i}"], lin[f"k{i}"]
    for kern, want in ((k, lin[f"A{i}"]), (k.conj().T, lin[f"AT{i}"])):
        got = cv.convolve(x, np.ascontiguousarray(kern), normalization_zero_tol=1e-4)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(f"case {i} {kern.shape}: {err:.2e} of the maximum")
        assert err < 1e-12


# ------------------------------------------------------- degrade, scale_psf
def test_degrade_is_the_references_call(cv):
    z = golden("app_subdiv_inputs.npz")
    img, psf = z["img"][100:170, 200:330], z["psf"]
    got = cv.degrade(img, psf)
    assert got.shape == (70, 130) and same(got, cv.convolve(img, psf, normalization_zero_tol=1e-4))
    assert same(got, conv_ref.convolve(img, psf))
    both = cv.degrade(np.stack([img, 2 * img]), np.stack([psf, psf[::-1].copy()]))
    assert same(both[0], got) and same(both[1], conv_ref.convolve(2 * img, psf[::-1]))
    with pytest.raises(ValueError, match="can't be normalized"):
        cv.degrade(img, psf * 1e-5)  # sum 1e-5 at tolerance 1e-4


def scale_bar(n):
    """Two orders of summing n positive terms differ by at most n * 2^-53 of the
    sum each side's error bound is (n - 1) * 2^-53 / 2 -- together n * 2^-53 --
    and the two divisions add 2^-53: (n + 2) * 2^-53 relative."""
    return (n + 2) * 2.0 ** -53


@pytest.mark.parametrize("shape", ((31, 31), (31, 25), (2, 31, 31)), ids=str)
def test_scale_psf(cv, shape):
    rng = np.random.default_rng(17)
    psf = seg_ref.make_kernel(4.0, 31)[..., :shape[-1]] * rng.uniform(0.9, 1.1, shape)
    kern = cv.make_2dgaussian_kernel(1.2, shape[-2:])
    assert kern.shape == tuple(shape[-2:])
    raw = cv.convolve(psf, kern)  # before the division: the restatement's bits
    want = np.stack([conv_ref.convolve(p, kern) for p in psf.reshape((-1,) + tuple(shape[-2:]))])
    assert same(raw.reshape(want.shape), want)
    got = cv.scale_psf(psf)
    n = shape[-2] * shape[-1]
    for g, w in zip(got.reshape(want.shape), want):
        ref = w / w.sum()
        assert np.max(np.abs(g - ref) / ref) <= scale_bar(n)
        assert abs(g.sum() - 1.0) <= scale_bar(n)
    assert same(cv.scale_psf(psf, 1.2, shape[-2:]), got)
    assert not same(cv.scale_psf(psf, 2.0), got)
