"""Time the source validation on the device: HIP
events, 2 warm-ups, median of 7.

The workload is the crowded 450 x 450 frame (tests/golden/crowded_inputs.npz)
and the catalogue source_info builds of it with n_pixels=1, as the
application's restored catalogues are built: 192 sources.  Timed one
call of bsgp_validate_sources each with preallocated outputs, reading the
catalogue's centroid columns in place, at window sizes 9, 31, 100 and 128, for
the frame alone and for a batch of 30 (the frame scaled by 1 + k / 100,
standing in for 30 candidate images); then the numpy restatement
(tests/validate_ref.py) of the same catalogue at size 100 on the host, and
source_info with and without validate=True.

    python tools/validate_timing.py --out profiles/validate/timing.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "beta-sgp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _bsgp as B  # noqa: E402
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
    with np.load(os.path.join(ROOT, "tests", "golden", "crowded_inputs.npz")) as z:
        img = np.ascontiguousarray(z["img"].astype(np.float32))  # stored big-endian
    H, W = img.shape
    L = B.lib()
    r = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "dtype": str(img.dtype)}
    for n in (1, a.images):
        frames = np.stack([img * np.float32(1.0 + k / 100.0) for k in range(n)])
        cat, bkg = S.source_info(frames, 60, 1, device_out=True)
        d = torch.from_numpy(frames).cuda()
        fc, cap = cat.f64_cols, cat.f64_cols.shape[1]
        nd = torch.from_numpy(np.asarray(cat.nlabels, dtype=np.int32)).cuda()
        stats = torch.empty((n, cap, 3), dtype=torch.float64, device="cuda")
        valid = torch.empty((n, cap), dtype=torch.int32, device="cuda")
        status = torch.empty((n, cap), dtype=torch.int32, device="cuda")
        xy = ctypes.c_void_p(fc.data_ptr() + 3 * 8)
        key = f"images_{n}"
        r[key] = {"sources_total": int(np.sum(cat.nlabels)), "cap": int(cap)}
        for size in (9, 31, 100, 128):
            def call():
                B.check(L.bsgp_validate_sources(
                    B._ptr(d), S._dtype(d), B._ptr(bkg.background), B._ptr(bkg.background_rms), n, H,
                    W, 1, xy, 8, B._ptr(nd), cap, size, size, 3.0, B._ptr(stats), B._ptr(valid),
                    B._ptr(status), B.current_stream()))
            t, allt = timed(call)
            k = int(nd[0])
            r[key][f"ms_validate_size_{size}"] = t
            r[key][f"ms_validate_size_{size}_all"] = allt
            r[key][f"valid_in_image_0_size_{size}"] = int(valid[0, :k].sum())
        for val in (False, True):
            t, _ = timed(lambda: S.source_info(frames, 60, 1, device_out=True, validate=val))
            r[key][f"ms_source_info_validate_{val}"] = t
        if n == 1:  # the host restatement of the same catalogue, size 100
            from validate_ref import validate_ref
            pos = np.stack([cat.xcentroid[0], cat.ycentroid[0]], axis=1)
            bg, rm = bkg.background[0].cpu().numpy(), bkg.background_rms[0].cpu().numpy()
            t0 = time.perf_counter()
            ref = validate_ref(img, pos, bg, rm, 100)
            r["ms_numpy_restatement_size_100_one_image"] = (time.perf_counter() - t0) * 1e3
            B.check(L.bsgp_validate_sources(
                B._ptr(d), S._dtype(d), B._ptr(bkg.background), B._ptr(bkg.background_rms), 1, H, W,
                1, xy, 8, B._ptr(nd), cap, 100, 100, 3.0, B._ptr(stats), B._ptr(valid),
                B._ptr(status), B.current_stream()))
            k = len(pos)
            r["device_equals_restatement"] = bool(
                np.array_equal(stats[0, :k].cpu().numpy(), ref["stats"], equal_nan=True)
                and np.array_equal(valid[0, :k].cpu().numpy() != 0, ref["valid"]))
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
