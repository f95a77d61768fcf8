"""Deblending of parents over the LDS cap on the device
(``deblend_sources(..., large_parents=True)``, ``bsgp_deblend_sources_large``,
``k_deblend_large``; DESIGN §3.8 "Parents over the LDS cap").

Every check of a label image is equality pixel for pixel: against the
skimage-pinned fixture deblend_cases.npz with every parent sent through the
global-memory kernel (``lds_max_box=0``), against deblend_large_cases.npz (two
real over-cap parents of the crowded frame) and against tests/deblend_ref.py,
which raises ``MarginError`` where an input is not tie-free by 1e-9 (values,
thresholds, flux fractions), so the expected images do not depend on the last
bits of the device's pow, sums or background map.  Synthetic inputs take the
first seed the restatement accepts.

The one float bar, for the sum of segment_flux with and without deblending, is
test_gpu_deblend.py's: §3.8's per-segment bar 2 * area * 2^-53 * sum|v| summed
over the undeblended segments, the totals taken with math.fsum.
"""
import math
import warnings

import numpy as np
import pytest
from scipy import ndimage

import deblend_ref
from conftest import golden

pytestmark = pytest.mark.gpu

CROPS = (3, 5, 438, 417, 47)
PARAMS = {"linear": dict(mode="linear"), "nlev1": dict(nlevels=1), "nlev8": dict(nlevels=8),
          "contrast0": dict(contrast=0.0), "contrast1": dict(contrast=1.0)}
GLOBAL = dict(large_parents=True, lds_max_box=0)  # every parent through k_deblend_large


@pytest.fixture(scope="module")
def sg():
    import _bsgp
    _bsgp.require_gpu()
    import segmentation
    return segmentation


@pytest.fixture(scope="module")
def fx():
    return golden("deblend_cases.npz")


@pytest.fixture(scope="module")
def big():
    return golden("deblend_large_cases.npz")


@pytest.fixture(scope="module")
def seg():
    return golden("seg_cases.npz")


@pytest.fixture(scope="module")
def crowded(sg):
    """The crowded frame's undeblended catalogue on the device, its maps on the
    host and its labels over the LDS cap."""
    img = golden("crowded_inputs.npz")["img"]
    plain = sg.source_info(img, 60, 5)[0]
    box = ((plain.bbox_xmax - plain.bbox_xmin + 1).astype(np.int64)
           * (plain.bbox_ymax - plain.bbox_ymin + 1))
    over = [int(l) for l in np.flatnonzero((box > sg.DEBLEND_MAX_BOX) & (plain.area >= 10)) + 1]
    return img, plain, over


def check(got, fx, tag):
    want = fx[f"{tag}_out"].astype(np.int32)
    assert got.data.dtype == np.int32 and got.data.shape == want.shape
    assert np.array_equal(got.data, want), (tag, int((got.data != want).sum()))
    assert got.nlabels == int(want.max())
    assert np.array_equal(got.parent, fx[f"{tag}_parent"][1:]), tag


def quiet(f, *a, **kw):
    """f(*a, **kw) with every warning an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return f(*a, **kw)


def blobs(shape, seed, nblob, noise=0.3):
    rng = np.random.default_rng(seed)
    H, W = shape
    yy, xx = np.mgrid[:H, :W]
    d = 5.0 + rng.normal(0.0, noise, shape)
    for _ in range(nblob):
        y0, x0 = rng.uniform(0, H - 1), rng.uniform(0, W - 1)
        amp, wid = rng.uniform(20.0, 60.0), rng.uniform(1.6, 3.0)
        d += amp * np.exp(-((yy - y0) ** 2 + (xx - x0) ** 2) / (2 * wid ** 2))
    return d


def first_accepted(make, lab, npixels, need_split=(), **kw):
    """(data, restatement's result) for the first seed whose data the
    restatement accepts as tie-free and that splits the parents need_split."""
    for seed in range(20):
        d = make(seed)
        try:
            ref, par, st = deblend_ref.deblend(d, lab, npixels, **kw)
        except deblend_ref.MarginError:
            continue
        if all((par[1:] == l).sum() > 1 for l in need_split):
            return d, ref, par
    raise AssertionError("no seed accepted")


def same_children(a, b, m):
    """The label images a and b split the pixels m the same way, in the same order."""
    pairs = np.unique(np.stack([a[m], b[m]]), axis=1)
    return (len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))
            and bool((np.diff(pairs[1]) > 0).all()))


# ---------------------------------------------------- 1: the pinned fixture
@pytest.mark.parametrize("tag", ("s1", "s2"))
def test_global_path_synthetic_fields(sg, fx, seg, tag):
    got = quiet(sg.deblend_sources, seg[f"{tag}_conv"], seg[f"{tag}_lab5"], 5, **GLOBAL)
    check(got, fx, tag)
    assert got.status == 0


@pytest.mark.parametrize("l", CROPS)
def test_global_path_application_parents(sg, fx, l):
    got = quiet(sg.deblend_sources, fx[f"crop{l}_conv"], fx[f"crop{l}_mask"].astype(np.int32), 1,
                **GLOBAL)
    check(got, fx, f"crop{l}")


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_global_path_parameters(sg, fx, seg, name):
    check(sg.deblend_sources(seg["s1_conv"], seg["s1_lab5"], 5, **PARAMS[name], **GLOBAL), fx,
          f"s1_{name}")
    got = sg.deblend_sources(fx["crop5_conv"], fx["crop5_mask"].astype(np.int32), 1, **PARAMS[name],
                             **GLOBAL)
    check(got, fx, f"crop5_{name}")


def test_global_path_connectivity_4(sg, fx, seg):
    got = sg.deblend_sources(seg["s1_conv"], fx["s1_lab1_conn4"], 1, connectivity=4, **GLOBAL)
    check(got, fx, "s1_conn4")
    got = sg.deblend_sources(fx["crop5_conv"], fx["crop5_lab_conn4"], 1, connectivity=4, **GLOBAL)
    check(got, fx, "crop5_conn4")


# ---------------------------------------------------- 2: real large parents
@pytest.mark.parametrize("tag", ("big", "small"))
def test_real_large_parents(sg, big, tag):
    import _bsgp
    d, m = big[f"{tag}_conv"], big[f"{tag}_mask"].astype(np.int32)
    assert m.size > sg.DEBLEND_MAX_BOX
    got = quiet(sg.deblend_sources, d, m, 5, large_parents=True)
    check(got, big, tag)
    assert got.status == 0 and got.nlabels > 1
    with pytest.warns(sg.DeblendBoxWarning, match="1 parent"):  # the default: as before
        left = sg.deblend_sources(d, m, 5)
    assert left.nlabels == 1 and np.array_equal(left.data, m) and list(left.parent) == [1]
    assert left.status == _bsgp.BSGP_DEBLEND_OVER_CAP


# ---------------------------------------------------- 3: the crowded frame
def test_crowded_frame_large_parents_against_the_restatement(sg, crowded):
    img, plain, over = crowded
    assert len(over) >= 2
    conv, lab = plain.convolved_data, plain.segment_img.data
    ref, par, st = deblend_ref.deblend(conv, lab, 5, labels=over)  # MarginError on a tie
    got = quiet(sg.deblend_sources, conv, plain.segment_img, 5, labels=over, large_parents=True)
    print(f"{plain.nlabels} parents, {len(over)} over the cap -> {st['nchildren']} children of "
          f"{st['nsplit']}; margins {st['gap']:.1e} {st['thr']:.1e} {st['frac']:.1e}")
    assert np.array_equal(got.data, ref), int((got.data != ref).sum())
    assert got.nlabels == int(ref.max()) and np.array_equal(got.parent, par[1:])
    assert got.status == 0 and st["nsplit"] >= 2


def test_crowded_frame_end_to_end(sg, crowded):
    img, plain, over = crowded
    deb = quiet(sg.source_info, img, 60, 5, deblend=True, large_parents=True)[0]
    assert deb.segment_img.status == 0  # no parent left over the cap
    with pytest.warns(sg.DeblendBoxWarning, match=f"{len(over)} parent"):
        capped = sg.source_info(img, 60, 5, deblend=True)[0]
    assert deb.nlabels > capped.nlabels > plain.nlabels
    assert len(deb) == deb.nlabels and int(plain.area.sum()) == int(deb.area.sum())
    lab, sub = plain.segment_img.data, plain.data
    bar = sum(2.0 * a * 2.0 ** -53 * s for a, s in
              zip(plain.area, ndimage.sum(np.abs(sub), lab, np.arange(1, plain.nlabels + 1))))
    diff = abs(math.fsum(deb.segment_flux) - math.fsum(plain.segment_flux))
    print(f"labels {plain.nlabels} -> {capped.nlabels} (cap) -> {deb.nlabels}; "
          f"|sum flux deblended - plain| = {diff:.3e}, bar {bar:.3e}")
    assert diff <= bar
    # the parents under the cap get what they got before
    small = ~np.isin(lab, over) & (lab > 0)
    assert same_children(deb.segment_img.data, capped.segment_img.data, small)


# ---------------------------------------------------- 4: path independence
def test_both_kernels_agree_on_ties(sg):
    """test_gpu_deblend.py's integer-valued plateau image (case 6), under the
    cap: the two kernels break every tie alike, twice."""
    yy, xx = np.mgrid[:18, :26]
    d = np.zeros((18, 26))
    for y0, x0, amp in ((5, 6, 9), (11, 17, 7), (4, 20, 5)):
        d += amp * np.exp(-((yy - y0) ** 2 + (xx - x0) ** 2) / 14.0)
    d = np.floor(d) + 1.0
    lab = np.ones(d.shape, np.int32)
    lab[0, :3] = 0
    for mode in ("linear", "exponential"):
        lds = sg.deblend_sources(d, lab, 2, mode=mode)
        glob = sg.deblend_sources(d, lab, 2, mode=mode, **GLOBAL)
        again = sg.deblend_sources(d, lab, 2, mode=mode, **GLOBAL)
        assert lds.nlabels >= 2
        assert np.array_equal(glob.data, lds.data) and glob.nlabels == lds.nlabels
        assert np.array_equal(glob.data, again.data)


# ---------------------------------------------------- 5: one row over the cap
def test_66_rows_of_64_just_over_the_cap(sg):
    lab = np.ones((66, 64), np.int32)
    assert lab.size - 2 * 64 == sg.DEBLEND_MAX_BOX
    d, ref, par = first_accepted(lambda s: np.random.default_rng(s).uniform(1.0, 2.0, lab.shape),
                                 lab, 2, need_split=(1,))
    got = quiet(sg.deblend_sources, d, lab, 2, large_parents=True)
    assert np.array_equal(got.data, ref) and np.array_equal(got.parent, par[1:])
    assert got.status == 0 and got.nlabels == int(ref.max()) > 100  # several passes of D6


# ---------------------------------------------------- 6: the shared workspace
def interlocking():
    lab = np.zeros((80, 80), np.int32)
    lab[2:78, 2:14], lab[66:78, 2:62] = 1, 1     # an L
    lab[2:14, 18:78], lab[2:78, 66:78] = 2, 2    # a turned L; each box holds the other's arm
    lab[18:62, 18:30], lab[50:62, 18:62] = 1, 1  # and arms inside each other's corner
    return lab


def ring():
    lab = np.zeros((76, 74), np.int32)
    lab[3:73, 2:72] = 1
    lab[15:61, 14:60] = 0
    lab[22:54, 21:53] = 2  # inside the hole; its box is under the cap
    return lab


@pytest.mark.parametrize("name,make,lds", (("interlocking", interlocking, None),
                                           ("ring", ring, None), ("ring", ring, 0)))
def test_parents_with_overlapping_boxes(sg, name, make, lds):
    lab = make()
    for l in (1, 2):
        ys, xs = np.nonzero(lab == l)
        size = (np.ptp(ys) + 1) * (np.ptp(xs) + 1)
        assert (size > sg.DEBLEND_MAX_BOX) == (l == 1 or name == "interlocking")
    kw = dict(large_parents=True) if lds is None else dict(large_parents=True, lds_max_box=lds)
    d, ref, par = first_accepted(lambda s: blobs(lab.shape, s, 40), lab, 5, need_split=(1, 2))
    got = quiet(sg.deblend_sources, d, lab, 5, **kw)
    assert np.array_equal(got.data, ref) and np.array_equal(got.parent, par[1:])
    for l in (1, 2):  # what each gets alone
        alone = quiet(sg.deblend_sources, d, (lab == l).astype(np.int32), 5, **kw)
        assert same_children(got.data, alone.data, lab == l), l
        assert np.array_equal(alone.data != 0, lab == l)


@pytest.mark.parametrize("shape", ((1, 5000), (5000, 1), (70, 70)))
def test_rows_columns_and_all_four_borders(sg, shape):
    lab = np.ones(shape, np.int32)

    def make(seed):
        if min(shape) > 1:
            return blobs(shape, seed, 12)
        x = np.arange(max(shape), dtype=np.float64)
        rng = np.random.default_rng(seed)
        d = 5.0 + rng.normal(0.0, 0.3, x.size)
        for _ in range(25):
            d += rng.uniform(20.0, 60.0) * np.exp(-(x - rng.uniform(0, x.size)) ** 2 / 18.0)
        return d.reshape(shape)

    d, ref, par = first_accepted(make, lab, 5, need_split=(1,))
    got = quiet(sg.deblend_sources, d, lab, 5, large_parents=True)
    assert np.array_equal(got.data, ref) and np.array_equal(got.parent, par[1:])
    assert got.status == 0


def test_connectivity_4_leaves_an_unreachable_pixel(sg):
    lab = np.ones((70, 70), np.int32)
    lab[0, 1] = lab[1, 0] = 0  # (0, 0) hangs on (1, 1) by its corner only
    d, ref, par = first_accepted(lambda s: blobs(lab.shape, s, 12), lab, 2, need_split=(1,),
                                 connectivity=4)
    assert ref[0, 0] == 0 and ref[1, 1] > 0
    got = quiet(sg.deblend_sources, d, lab, 2, connectivity=4, large_parents=True)
    assert np.array_equal(got.data, ref) and got.data[0, 0] == 0
    assert np.array_equal(got.parent, par[1:])


# ---------------------------------------------------- 7: batches
def test_batch_equals_single_images(sg, fx, big):
    """Small parents only, a large parent, no labels, both kinds: every image
    gets what it gets alone, twice; labels= reaches a large parent."""
    H, W = 112, 120
    data, labs = np.zeros((4, H, W)), np.zeros((4, H, W), np.int32)

    def put(b, d, m, y, x, l):
        h, w = d.shape
        data[b, y:y + h, x:x + w] = np.where(m, d, data[b, y:y + h, x:x + w])
        labs[b, y:y + h, x:x + w] = np.where(m, l, labs[b, y:y + h, x:x + w])

    put(0, fx["crop3_conv"], fx["crop3_mask"], 0, 0, 1)
    put(0, fx["crop5_conv"], fx["crop5_mask"], 40, 50, 2)
    put(1, big["big_conv"], big["big_mask"], 0, 0, 1)
    put(3, big["small_conv"], big["small_mask"], 0, 0, 1)
    put(3, fx["crop3_conv"], fx["crop3_mask"], 70, 85, 2)
    got = quiet(sg.deblend_sources, data, labs, 5, large_parents=True)
    again = sg.deblend_sources(data, labs, 5, large_parents=True)
    assert np.array_equal(got.data, again.data) and np.array_equal(got.nlabels, again.nlabels)
    assert list(got.status) == [0, 0, 0, 0]
    assert got.nlabels[2] == 0 and not got.data[2].any() and len(got.parent[2]) == 0
    for b in (0, 1, 3):
        one = sg.deblend_sources(data[b], labs[b], 5, large_parents=True)
        assert np.array_equal(got.data[b], one.data) and got.nlabels[b] == one.nlabels, b
        assert np.array_equal(got.parent[b], one.parent)
    h, w = big["big_out"].shape
    assert np.array_equal(got.data[1, :h, :w], big["big_out"])
    h, w = big["small_out"].shape
    m = big["small_mask"]
    assert same_children(got.data[3, :h, :w], big["small_out"].astype(np.int32), m)
    # labels=: the large parent alone; the other stays one segment, in front
    sel = quiet(sg.deblend_sources, data[3], labs[3], 5, labels=[1], large_parents=True)
    assert np.array_equal(sel.data == 1, labs[3] == 2) and list(sel.parent[:1]) == [2]
    assert sel.nlabels == 1 + int(big["small_out"].max())
    assert np.array_equal(sel.data[:h, :w][m] - 1, big["small_out"][m])


# ---------------------------------------------------- 8: the area bound
def test_parent_over_the_area_bound_is_left_and_reported(sg):
    import _bsgp
    H, W = 513, 512
    assert H * W > sg.DEBLEND_LARGE_MAX_AREA >= (H - 1) * W
    d = np.random.default_rng(3).uniform(1.0, 2.0, (H, W))
    lab = np.ones((H, W), np.int32)
    with pytest.warns(sg.DeblendBoxWarning, match=f"1 parent.*{sg.DEBLEND_LARGE_MAX_AREA}.*area limit"):
        got = sg.deblend_sources(d, lab, 5, large_parents=True)
    assert got.nlabels == 1 and list(got.parent) == [1]
    assert got.status == _bsgp.BSGP_DEBLEND_OVER_CAP
    assert np.array_equal(got.data, lab)
    # not selected: not reported
    two = lab.copy()
    two[10:14, 10:14] = 2
    sel = quiet(sg.deblend_sources, d, two, 1, labels=[2], nlevels=2, large_parents=True)
    assert sel.status == 0 and np.array_equal(sel.data == 1, two == 1)
