"""Generate tests/golden/deblend_large_cases.npz: parents whose bounding box is
over the LDS cap of the device deblending (``DEBLEND_MAX_BOX`` = 4096 box
pixels), for ``deblend_sources(..., large_parents=True)`` (DESIGN §3.8,
"Parents over the LDS cap").

The inputs are crops of the crowded 450 x 450 frame (crowded_inputs.npz):
``img - bkg`` convolved with tests/seg_ref.py's kernel and ``convolve``,
detected with ``seg_ref.detect`` at 1.5 x a sigma-clipped rms and npixels 5;
of the detected parents over the cap, the one with the largest and the one
with the smallest box.  ``(conv crop, mask)`` is stored as an input in its own
right, as the ``crop{l}`` cases of deblend_cases.npz are.  The expected label
images come from tests/deblend_ref.py (steps D1 to D7) with its serial flood:
scikit-image is not available where this file is generated.  The generator
asserts deblend_ref's three tie margins of 1e-9 (values, thresholds, flux
fractions); with those, skimage's insertion-age rule and the index rule of the
serial flood coincide, as make_golden_deblend.py established for its cases by
running both.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_deblend_large.py
"""
import os
import sys

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import numpy as np  # noqa: E402

import deblend_ref as ref  # noqa: E402
import seg_ref  # noqa: E402

MAX_BOX = 4096
NPIXELS = 5


def clipped_rms(a, sigma=3.0, iters=10):
    """Standard deviation after clipping at sigma standard deviations around the median."""
    v = np.asarray(a, dtype=np.float64).ravel()
    for _ in range(iters):
        med, sd = np.median(v), v.std()
        keep = np.abs(v - med) <= sigma * sd
        if keep.all():
            break
        v = v[keep]
    return float(v.std())


def main():
    with np.load(os.path.join(OUT, "crowded_inputs.npz")) as f:
        sub = f["img"].astype(np.float64) - f["bkg"]
    conv = seg_ref.convolve(sub, seg_ref.make_kernel(1.2, 3))
    rms = clipped_rms(sub)
    lab, n = seg_ref.detect(conv, 1.5 * rms, NPIXELS)
    boxes = {}
    for l in range(1, n + 1):
        yy, xx = np.nonzero(lab == l)
        sl = (slice(yy.min(), yy.max() + 1), slice(xx.min(), xx.max() + 1))
        size = (sl[0].stop - sl[0].start) * (sl[1].stop - sl[1].start)
        if size > MAX_BOX and len(yy) >= 2 * NPIXELS:
            boxes[l] = (size, sl)
    assert len(boxes) >= 2, boxes
    order = sorted(boxes, key=lambda l: boxes[l][0])
    z = {"rms": np.float64(rms)}
    print(f"rms {rms:.6g}, {n} segments, {len(boxes)} over the cap: "
          f"{sorted(b[0] for b in boxes.values())}")
    for tag, l in (("big", order[-1]), ("small", order[0])):
        sl = boxes[l][1]
        mask = lab[sl] == l
        d = conv[sl]
        out, parent, st = ref.deblend(d, mask.astype(np.int32), NPIXELS)  # asserts the margins
        assert st["nsplit"] == 1 and mask.size > MAX_BOX
        z[f"{tag}_conv"], z[f"{tag}_mask"] = d, mask
        z[f"{tag}_out"], z[f"{tag}_parent"] = out.astype(np.int16), parent
        print(f"  {tag}: label {l}, box {mask.shape} = {mask.size}, area {int(mask.sum())}, "
              f"children {st['nchildren']}, region replacements {st['splits']}, removals "
              f"{st['removals']}, margins gap {st['gap']:.2e} thr {st['thr']:.2e} frac {st['frac']:.2e}")
    path = os.path.join(OUT, "deblend_large_cases.npz")
    np.savez_compressed(path, **z)
    print("deblend_large_cases.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
