"""Time the local background of the source catalogue
on the device: HIP events, 2 warm-ups, median of 7.

The workload is the batch the multistart score evaluates: 30 candidate tiles
of 375 x 375.  The tiles are the frame tests/golden/SUBDIV_ORIGIMG.fits scaled
by 1 + k / 100 (k = 0..29), which stand in for 30 restored candidates of one
subdivision; they hold about 100 sources each.  Timed one call each with
preallocated outputs: bsgp_segment_catalog and, next to it,
bsgp_segment_local_background (width 5, sigma 3, 10 iterations, 10 values;
apply = 0, so that repeated calls do not keep correcting the same columns: the
correction itself is three stores per source) on the deblended labels of
source_info; then source_info as a whole with and without the width, with and
without deblending.  The annulus sizes say which of the kernel's two launches
(16 KiB and 64 KiB of LDS) served the sources.

    python tools/localbkg_timing.py --out profiles/localbkg/timing.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "beta-sgp_amd"))

import _bsgp as B  # noqa: E402
import fits_io  # noqa: E402
import segmentation as S  # noqa: E402

torch = B.torch


def timed(fn, warm=2, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [float(m) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=30)
    a = ap.parse_args()
    B.require_gpu()
    _, img = fits_io.read_fits(os.path.join(ROOT, "tests", "golden", "SUBDIV_ORIGIMG.fits"))
    n = a.images
    tiles = np.stack([img * np.float32(1.0 + k / 100.0) for k in range(n)])
    H, W = img.shape
    L = B.lib()
    cat, _ = S.source_info(tiles, 60, 5, deblend=True, device_out=True, localbkg_width=5)
    sub, conv, lab = cat.data, cat.convolved_data, cat.segment_img.data
    ic, cap = cat.int_cols, cat.int_cols.shape[1]
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    nlab = torch.from_numpy(np.asarray(cat.nlabels, dtype=np.int32)).cuda()
    ic2, fc2, cst = torch.empty((n, cap, 5), **i32), torch.empty((n, cap, 8), **f64), torch.empty((n,), **i32)
    lb, npx, lst = torch.empty((n, cap), **f64), torch.empty((n, cap, 2), **i32), torch.empty((n,), **i32)
    s = B.current_stream

    def measure():
        B.check(L.bsgp_segment_catalog(B._ptr(sub), B._ptr(conv), B._ptr(lab), n, H, W, cap,
                                       B._ptr(nlab), B._ptr(ic2), B._ptr(fc2), B._ptr(cst), s()))

    def local(width=5.0):
        B.check(L.bsgp_segment_local_background(
            B._ptr(sub), B.BSGP_DTYPE_F64, B._ptr(lab), n, H, W, cap, B._ptr(nlab), B._ptr(ic), None,
            width, 3.0, 10, 10, 0, B._ptr(lb), B._ptr(npx), B._ptr(lst), s()))

    t_cat, t_cat_all = timed(measure)
    t_lb, t_lb_all = timed(local)
    assert torch.equal(lb, cat.local_background_dev)
    gathered = npx[:, :, 0].cpu().numpy()
    gathered = gathered[gathered > 0]
    t_lb20, _ = timed(lambda: local(20.0))
    big20 = npx[:, :, 0].cpu().numpy()
    r = {"device": torch.cuda.get_device_name(0), "images": n, "H": H, "W": W, "cap": cap,
         "sources_total": int(np.sum(cat.nlabels)), "sources_max_per_image": int(np.max(cat.nlabels)),
         "annulus_values_median": float(np.median(gathered)), "annulus_values_max": int(gathered.max()),
         "sources_with_more_than_2048_annulus_values": int((gathered > 2048).sum()),
         "ms_segment_catalog": t_cat, "ms_segment_catalog_all": t_cat_all,
         "ms_segment_local_background": t_lb, "ms_segment_local_background_all": t_lb_all,
         "ms_segment_local_background_width_20": t_lb20,
         "annulus_values_max_width_20": int(big20.max())}
    for deb in (False, True):
        for width in (0, 5):
            t, allt = timed(lambda: S.source_info(tiles, 60, 5, deblend=deb, device_out=True,
                                                  localbkg_width=width))
            r[f"ms_source_info_deblend_{deb}_localbkg_width_{width}"] = t
            r[f"ms_source_info_deblend_{deb}_localbkg_width_{width}_all"] = allt
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
