"""Time the star-stamp metrics on the device: HIP events around
the calls, 2 warm-ups, median of 7.

The workload is the batch bench.py --config stamps31 solves: 16384 float32
stamps of 31 x 31, here a Gaussian star on noise as the observed stamp and a
narrower one as the restored stamp, centres within half a pixel of the
middle.  Timed: each kernel through its C-ABI call with preallocated outputs
(bsgp_radial_profile, bsgp_fit_gauss1d, bsgp_wasserstein1: one call each, of
the observed stamps), then stamps.stamp_metrics as a user calls it (two profile
calls, two fits, one distance, with its allocations and the copies of the
centres and FWHMs).  Each kernel is put beside a device-to-device copy of the
bytes it reads, and the whole beside the same work with numpy and scipy on the
host (tests/stamps_ref.py), a subset timed and scaled to the batch.

    python tools/stamp_metrics_timing.py --out profiles/stampmetrics/timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "beta-sgp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _bsgp as B  # noqa: E402
import stamps as S  # noqa: E402

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


def copy_ms(nbytes):
    src = torch.empty(max(1, int(nbytes)), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src))[0]


def stars(rng, n, size, sigma, amp):
    """n stamps: a Gaussian of width sigma[i] about a centre near the middle on
    noise of sigma 1; returns (float32 stamps, centres [n, 2], FWHMs [n])."""
    c = (size - 1) / 2.0 + rng.uniform(-0.5, 0.5, (n, 2))
    ii, jj = np.mgrid[:size, :size]
    r2 = (ii[None] - c[:, 0, None, None]) ** 2 + (jj[None] - c[:, 1, None, None]) ** 2
    d = amp[:, None, None] * np.exp(-0.5 * r2 / sigma[:, None, None] ** 2)
    d += rng.normal(0.0, 1.0, d.shape)
    return d.astype(np.float32), c, 2.0 * np.sqrt(2.0 * np.log(2.0)) * sigma


def host_metrics(o, r, co, cr, fo, fr):
    import stamps_ref as R
    out = []
    for k in range(len(o)):
        fa = R.fit_gauss1d(R.radial_profile(o[k].astype(np.float64), co[k]), fo[k])
        fb = R.fit_gauss1d(R.radial_profile(r[k].astype(np.float64), cr[k]), fr[k])
        out.append(R.wasserstein1(fa["fitted"], fb["fitted"])[0])
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--host-stamps", type=int, default=128)
    a = ap.parse_args()
    B.require_gpu()
    rng = np.random.default_rng(0)
    n, size = a.batch, 31
    o, co, fo = stars(rng, n, size, rng.uniform(1.3, 2.0, n), rng.uniform(50.0, 2000.0, n))
    r, cr, fr = stars(rng, n, size, rng.uniform(0.7, 1.2, n), rng.uniform(200.0, 8000.0, n))
    L = B.lib()
    s = B.current_stream
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    od, rd = torch.from_numpy(o).cuda(), torch.from_numpy(r).cuda()
    cod, fod = torch.from_numpy(co).cuda(), torch.from_numpy(fo).cuda()
    rcap = max(S.check_profile_args(o.shape, co)[2], S.check_profile_args(r.shape, cr)[2])
    prof, length = torch.empty((n, rcap), **f64), torch.empty((n,), **i32)
    fitted, params, perr = torch.empty((n, rcap), **f64), torch.empty((n, 3), **f64), \
        torch.empty((n, 3), **f64)
    info, wd = torch.empty((n, 2), **i32), torch.empty((n,), **f64)

    def profile():
        B.check(L.bsgp_radial_profile(B._ptr(od), B.BSGP_DTYPE_F32, n, size, size, B._ptr(cod), rcap,
                                      B._ptr(prof), B._ptr(length), s()))

    def fit():
        B.check(L.bsgp_fit_gauss1d(B._ptr(prof), B._ptr(length), n, rcap, B._ptr(fod),
                                   B._ptr(fitted), B._ptr(params), B._ptr(perr), B._ptr(info), s()))

    def w1():
        B.check(L.bsgp_wasserstein1(B._ptr(fitted), B._ptr(length), B._ptr(prof), B._ptr(length), n,
                                    rcap, B._ptr(wd), s()))

    t_prof, _ = timed(profile)
    t_fit, _ = timed(fit)
    t_w1, _ = timed(w1)
    t_all, t_all_all = timed(lambda: S.stamp_metrics(od, rd, co, cr, fo, fr, device_out=True))
    res = S.stamp_metrics(od, rd, co, cr, fo, fr)
    nfev = res["nfev"]
    read = {"radial_profile": n * size * size * 4 + n * 16, "fit_gauss1d": n * rcap * 8 + n * 12,
            "wasserstein1": 2 * n * rcap * 8 + n * 8}
    copies = {k: copy_ms(v) for k, v in read.items()}
    copies["all_five_calls"] = copy_ms(2 * read["radial_profile"] + 2 * read["fit_gauss1d"]
                                       + read["wasserstein1"])
    h = min(a.host_stamps, n)
    t0 = time.perf_counter()
    host_wd = host_metrics(o[:h], r[:h], co[:h], cr[:h], fo[:h], fr[:h])
    host_s = time.perf_counter() - t0
    out = {
        "device": torch.cuda.get_device_name(0), "stamps": n, "H": size, "W": size,
        "input": "float32", "rcap": rcap,
        "ms_radial_profile_one_call": t_prof, "ms_fit_gauss1d_one_call": t_fit,
        "ms_wasserstein1_one_call": t_w1,
        "ms_stamp_metrics_five_calls": t_all, "ms_stamp_metrics_all": t_all_all,
        "bytes_read": read, "ms_d2d_copy_of_the_bytes_read": copies,
        "nfev_mean": float(nfev.mean()), "nfev_max": int(nfev.max()),
        "fits_ended_on_maxfev": int((res["ier"] == 5).sum()),
        "host_numpy_scipy_s": host_s, "host_stamps": h,
        "host_s_scaled_to_all_stamps": host_s * n / h,
        "wd_device_vs_host_max_rel": float(np.nanmax(np.abs(res["wd"][:h] - host_wd)
                                                     / np.abs(host_wd))),
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
