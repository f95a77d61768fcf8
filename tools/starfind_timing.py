"""Time star finding on the device: HIP events around each of
the four C-ABI calls (bsgp_star_maps, bsgp_star_peaks, bsgp_star_measure,
bsgp_star_select) on inputs already on the device (the outputs come from
torch's caching allocator inside the timed region, as find_stars takes them),
2 warm-ups, median of 7.

Shapes: the crowded 450 x 450 frame of tests/golden/crowded_inputs.npz alone
and as a batch of 30, fwhm 4.5, the noise 1.4826 times the median absolute
deviation of the frame minus its background map.  The numpy restatement
(tests/starfind_ref.py) on the host, one frame, is put beside them.

    python tools/starfind_timing.py --out profiles/starfind/timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("beta-sgp_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))

SHAPES = [("frame", 1), ("batch_30", 30)]
FWHM = 4.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import _bsgp as B
    import segmentation as S
    import starfind as sf
    import starfind_ref as R
    torch = B.torch
    B.require_gpu()

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
        return float(np.median(ms)), [round(float(m), 4) for m in ms]

    with np.load(os.path.join(ROOT, "tests", "golden", "crowded_inputs.npz")) as z:
        img, bkg = np.ascontiguousarray(z["img"]), np.asarray(z["bkg"], dtype=np.float64)
    img = img.astype(img.dtype.newbyteorder("="))
    resid = img.astype(np.float64) - bkg
    noise = float(1.4826 * np.median(np.abs(resid - np.median(resid))))
    res = {"fwhm": FWHM, "noise": noise, "shapes": {}}

    t0 = time.perf_counter()
    want = R.find_stars(img, FWHM, noise)
    t_find = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    R.select_psf_stars(want["x"], want["y"], want["flux"], want["peak"], want["nsat"],
                       want["status"], img.shape, fwhm=FWHM)
    t_sel = (time.perf_counter() - t0) * 1e3
    res["numpy_restatement_ms"] = {"find_stars": t_find, "select_psf_stars": t_sel}
    res["candidates"] = int(len(want["ic"]))
    res["kept"] = int(((want["status"] & R.REJECTED) == 0).sum())
    print(f"numpy restatement, one frame: find_stars {t_find:.1f} ms, select {t_sel:.2f} ms; "
          f"{res['candidates']} candidates, {res['kept']} kept")

    for name, nb in SHAPES:
        imgs = np.broadcast_to(img, (nb,) + img.shape).copy()
        stars = sf.find_stars(imgs, FWHM, noise, device_out=True)
        assert np.array_equal(stars[0]["ic"], want["ic"]) and np.array_equal(stars[nb - 1]["status"],
                                                                              want["status"])
        c = sf.check_find_args(imgs.shape, FWHM)
        cs = sf.check_select_args(fwhm=FWHM)
        d, _ = S._to_dev(imgs)
        tp = sf.star_template(FWHM)
        t, halfw = sf._template_dev(tp)
        nz, nz_map = sf._noise_dev(noise, c)
        corr, amp = sf._maps_dev(d, None, t, halfw, c["R"], tp["tt"])
        peaks, nd, _ = sf._peaks_dev(d, corr, amp, t, halfw, tp["tt"], nz, nz_map, c)
        rows = max(1, int(nd.max()))
        peaks = peaks[:, :rows].contiguous()
        fcols, icols = sf._measure_dev(d, None, corr, amp, halfw, peaks, nd, c, None)
        row = {"B": nb, "H": img.shape[0], "W": img.shape[1], "stars": rows,
               "dtype": str(img.dtype), "support": tp["n"]}
        row["maps_ms"], row["maps_all_ms"] = timed(
            lambda: sf._maps_dev(d, None, t, halfw, c["R"], tp["tt"]))
        row["peaks_ms"], row["peaks_all_ms"] = timed(
            lambda: sf._peaks_dev(d, corr, amp, t, halfw, tp["tt"], nz, nz_map, c))
        row["measure_ms"], row["measure_all_ms"] = timed(
            lambda: sf._measure_dev(d, None, corr, amp, halfw, peaks, nd, c, None))
        row["select_ms"], row["select_all_ms"] = timed(
            lambda: sf._select_dev(fcols, icols, nd, img.shape, cs))
        t0 = time.perf_counter()
        sf.find_stars(imgs, FWHM, noise)
        row["find_stars_host_to_host_ms"] = (time.perf_counter() - t0) * 1e3  # with the copies
        res["shapes"][name] = row
        print(name, json.dumps({k: (round(v, 4) if isinstance(v, float) else v)
                                for k, v in row.items() if not k.endswith("all_ms")}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
