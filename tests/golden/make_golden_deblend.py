"""Generate tests/golden/deblend_cases.npz: inputs and expected outputs of the
device deblending (beta-sgp_amd/segmentation.py ``deblend_sources``, DESIGN
§3.8 "Deblending").

photutils is not available, so the expected label images come from the parts
its ``deblend_sources`` (1.5 to 1.8) is built from: the level components from
``scipy.ndimage.label`` and the flood from ``skimage.segmentation.watershed``
(scikit-image 0.18.3), put together as DESIGN §3.8 states the algorithm
(steps D1 to D7) by tests/deblend_ref.py, with skimage's watershed as its flood.  Run from the repository root with the interpreter
make_golden_seg.py uses (python 3.9):

    PYTHONDONTWRITEBYTECODE=1 python3.9 tests/golden/make_golden_deblend.py

The generator asserts, for every parent of every case, that
 1. no two pixels of the parent have equal data, and the smallest relative gap
    between two values is above MARGIN (deblend_ref.MARGIN, 1e-9);
 2. no pixel lies within MARGIN (relative) of a threshold t_k;
 3. no flux fraction lies within MARGIN (relative) of ``contrast`` and no two
    fractions below ``contrast`` lie within MARGIN of each other,
so that the expected labels do not depend on the last bits of the device's
``pow``, sums or background map, nor on how the flood breaks ties (skimage: by
insertion age; the device: by the smaller index).  A synthetic case that
violates one takes the next seed.
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deblend_ref as ref  # noqa: E402  (tests/deblend_ref.py: D1 to D7 in numpy and scipy)
import make_golden_bkg as gb  # noqa: E402
import make_golden_seg as gs  # noqa: E402
from deblend_ref import structure  # noqa: E402
from scipy import ndimage  # noqa: E402
from skimage.segmentation import watershed  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CROPS = (3, 5, 438, 417, 47)  # parents of the application tile's lab1


def skimage_flood(neg, markers, mask, connectivity):
    """skimage's watershed, asserted equal to the serial flood of D5 (the cases
    are tie-free, so the tie rules cannot differ)."""
    out = watershed(neg, markers, mask=mask, connectivity=connectivity)
    assert np.array_equal(out, ref.flood_serial(neg, markers, mask, connectivity))
    return out


def deblend(data, seg, npixels, **kw):
    try:
        out, parent, stats = ref.deblend(data, seg, npixels, flood=skimage_flood, **kw)
    except ref.MarginError as e:
        raise gb.MarginError(str(e))
    stats.pop("markers", None)
    return out, parent, stats


def blobs(shape, nblob, base, noise, width=1.6):
    def make(rng):
        H, W = shape
        yy, xx = np.mgrid[:H, :W]
        d = base + rng.normal(0.0, noise, shape)
        for _ in range(nblob):
            y0, x0, amp = rng.uniform(0, H - 1), rng.uniform(0, W - 1), rng.uniform(20.0, 60.0)
            d += amp * np.exp(-((yy - y0) ** 2 + (xx - x0) ** 2) / (2 * width ** 2))
        return d
    return make


def main():
    z, report = {}, {}

    def put(tag, out, parent, stats):
        z[f"{tag}_out"], z[f"{tag}_parent"] = out.astype(np.int16), parent
        report[tag] = {k: (float(f"{v:.2e}") if isinstance(v, float) else int(v))
                       for k, v in stats.items()}

    with np.load(os.path.join(OUT, "seg_cases.npz")) as f:
        seg = {k: f[k] for k in f.files}

    # case 1: s1 and s2 of seg_cases.npz, npixels 5, defaults
    for tag in ("s1", "s2"):
        put(tag, *deblend(seg[f"{tag}_conv"], seg[f"{tag}_lab5"], 5))

    # case 3 (and the crops of case 2): the application tile
    with np.load(os.path.join(OUT, "app_subdiv_inputs.npz")) as f:
        tile = f["img"]
    res = gs.case(tile, (60, 60), (5, 1))
    conv = res["conv"]
    assert np.array_equal(res["lab5"], seg["app_lab5"]) and np.array_equal(res["lab1"], seg["app_lab1"])
    for npix in (5, 1):
        put(f"app{npix}", *deblend(conv, res[f"lab{npix}"], npix))
    lab1 = res["lab1"].astype(np.int32)
    for l in CROPS:
        sl = ndimage.find_objects(lab1)[l - 1]
        m = lab1[sl] == l
        z[f"crop{l}_conv"], z[f"crop{l}_mask"] = conv[sl], m
        put(f"crop{l}", *deblend(conv[sl], m.astype(np.int32), 1))
        assert report[f"crop{l}"]["nsplit"] == 1

    # case 4: parameters, on s1 and on crop 5
    s1c4 = ndimage.label(seg["s1_conv"] > 1.5 * seg["s1_rms"],
                         structure=structure(4))[0].astype(np.int16)
    z["s1_lab1_conn4"] = s1c4
    c5 = z["crop5_conv"], z["crop5_mask"].astype(np.int32)
    for name, kw in (("linear", dict(mode="linear")), ("nlev1", dict(nlevels=1)),
                     ("nlev8", dict(nlevels=8)), ("contrast0", dict(contrast=0.0)),
                     ("contrast1", dict(contrast=1.0))):
        put(f"s1_{name}", *deblend(seg["s1_conv"], seg["s1_lab5"], 5, **kw))
        put(f"crop5_{name}", *deblend(c5[0], c5[1], 1, **kw))
    put("s1_conn4", *deblend(seg["s1_conv"], s1c4, 1, connectivity=4))
    m4 = ndimage.label(c5[1], structure=structure(4))[0].astype(np.int32)
    z["crop5_lab_conn4"] = m4.astype(np.int16)
    put("crop5_conn4", *deblend(c5[0], m4, 1, connectivity=4))
    # labels=: a subset of the parents; the others stay as they are
    def split_parents(tag):
        par = z[f"{tag}_parent"][1:]
        return sorted(set(int(p) for p in par if (par == p).sum() > 1))

    sp = split_parents("s1")
    n1 = int(seg["s1_lab5"].max())
    z["s1_subset_in"] = np.array(sp + [1 if 1 not in sp else 2], dtype=np.int32)
    z["s1_subset_out"] = np.array([l for l in range(1, n1 + 1) if l not in sp], dtype=np.int32)
    for name in ("subset_in", "subset_out"):
        put(f"s1_{name}r", *deblend(seg["s1_conv"], seg["s1_lab5"], 5, labels=list(z[f"s1_{name}"])))
    assert np.array_equal(z["s1_subset_inr_out"], z["s1_out"])
    assert np.array_equal(z["s1_subset_outr_out"], seg["s1_lab5"])
    sp = split_parents("app5")
    assert len(sp) >= 4
    z["app5_subset"] = np.array(sp[::2], dtype=np.int32)
    put("app5_subsetr", *deblend(conv, res["lab5"], 5, labels=sp[::2]))
    assert report["app5_subsetr"]["nsplit"] == len(sp[::2])

    # case 5: edges.  Whole images as one parent (it touches all four borders)
    def whole(tag, shape, nblob, shift=None, **kw):
        def ok(d):
            d = shifted(d)
            o, _, st = deblend(d, np.ones(shape, np.int32), 2, **kw)
            return st["nsplit"] == 1
        def shifted(d):
            if shift == "zero":
                return d - d.min()
            return d if shift is None else d - shift
        seed, d = gb.first_seed(blobs(shape, nblob, 5.0, 0.3), ok)
        d = shifted(d)
        z[f"{tag}_data"], z[f"{tag}_seed"] = d, seed
        put(tag, *deblend(d, np.ones(shape, np.int32), 2, **kw))
        return d

    whole("e_row", (1, 40), 3)
    whole("e_col", (40, 1), 3)
    whole("e_full", (12, 15), 3)
    d = whole("e_neg", (12, 15), 3, shift=9.0)
    assert d.min() < 0
    o_lin = deblend(d, np.ones(d.shape, np.int32), 2, mode="linear")[0]
    assert np.array_equal(o_lin, z["e_neg_out"])
    d = whole("e_zero", (12, 15), 3, shift="zero")
    assert d.min() == 0.0

    path = os.path.join(OUT, "deblend_cases.npz")
    np.savez_compressed(path, **z)
    print("deblend_cases.npz:", os.path.getsize(path), "bytes")
    for k, v in report.items():
        print(f"  {k}: {v}")


if __name__ == "__main__":
    main()
