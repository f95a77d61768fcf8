"""Time the star-stamp driver and its two kernels on the device.

* ``sgp_star_stamps`` on N positions of tests/golden/SUBDIV_ORIGIMG.fits: the
  bright pixels bench.py's ``stamp_inputs`` draws (the brightest 2 % of the
  frame's interior, with replacement, seed 0) plus a uniform sub-pixel offset
  in [-0.5, 0.5).  Host clock around the call (it returns host arrays, so it
  ends in a synchronisation), 1 warm-up, --reps runs; the solve's share is the
  device-event time the driver reports (EXEC_TIME times the kept stars).
* ``bsgp_extract_stamps`` and ``bsgp_stamp_select`` alone: HIP events around
  --launches back-to-back launches, 2 warm-ups, median of 7, outputs
  preallocated.  ``bsgp_extract_tiles`` moves the same number of float64 bytes
  from the same frame in the same run, as the yardstick.

    python tools/starstamps_timing.py --out profiles/starstamps/timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "beta-sgp_amd"), os.path.join(ROOT, "tests")]

import _bsgp as B  # noqa: E402
import fits_io  # noqa: E402
import stamps as S  # noqa: E402
import starstamps_ref as ref  # noqa: E402

torch = B.torch
BITS = {k: getattr(B, "BSGP_STAMP_" + k) for k in
        ("PARTIAL", "NO_OVERLAP", "BAD_POSITION", "NO_SOURCE", "MULTI_SOURCE", "BAD_FLUX",
         "NO_CANDIDATE", "RESTORED_NO_SOURCE")}


def timed(fn, launches, warm=2, reps=7):
    """Median ms per launch over reps windows of `launches` launches."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / launches)
    return float(np.median(ms)), [float(m) for m in ms]


def positions(img, n, seed=0):
    a = np.asarray(img, dtype=np.float32)
    inner = a[15:-15, 15:-15]
    rows, cols = np.nonzero(inner >= np.quantile(inner, 0.98))
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(rows), n)
    off = rng.uniform(-0.5, 0.5, (n, 2))
    return np.stack((cols[pick] + 15 + off[:, 0], rows[pick] + 15 + off[:, 1]), axis=1)


def driver(img, psf, pos, reps, maxit):
    runs = []
    res = None
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = S.sgp_star_stamps(img, pos, psf, MAXIT=maxit)
        dt = time.perf_counter() - t0
        nk = len(res["kept"])
        if i:  # (the first run warms the plans, the code objects and the allocator)
            runs.append({"s_total": dt, "s_solve": float(res["EXEC_TIME"][0]) * nk if nk else 0.0})
    tot = float(np.median([r["s_total"] for r in runs]))
    sol = float(np.median([r["s_solve"] for r in runs]))
    st = res["status"]
    fin = np.isfinite(res["WD_RADIAL_PROFILE_DISTANCE"])
    return {"positions": len(pos), "kept": int(len(res["kept"])), "candidates": int(res["scores"].shape[1]),
            "MAXIT": maxit, "runs": runs, "s_total_median": tot, "s_solve_median": sol,
            "fraction_outside_solve": (tot - sol) / tot,
            "stars_per_status_bit": {k: int(np.count_nonzero(st & v)) for k, v in BITS.items()},
            "iterations_of_the_winners_median": float(np.median(res["NUM_ITERS"])),
            "finite_wd": int(fin.sum()), "solver_status_any": int(np.any(res["solver_status"]))}


def kernels(img, pos, launches):
    out = {}
    n, sh, sw = len(pos), 31, 31
    xy = torch.from_numpy(pos).cuda()
    box, st = (torch.empty((n, 4), dtype=torch.int32, device="cuda"),
               torch.empty((n,), dtype=torch.int32, device="cuda"))
    H, W = img.shape
    for name, dt, code in (("f32", np.float32, B.BSGP_DTYPE_F32), ("f64", np.float64, B.BSGP_DTYPE_F64)):
        im = torch.from_numpy(np.ascontiguousarray(img, dtype=dt)).cuda()
        o = torch.empty((n, sh, sw), dtype=im.dtype, device="cuda")

        def cut():
            B.check(B.lib().bsgp_extract_stamps(B._ptr(im), code, H, W, B._ptr(xy), n, sh, sw, B._ptr(o),
                                                B._ptr(box), B._ptr(st), B.current_stream()))
        ms, allms = timed(cut, launches)
        want = ref.cutout_ref(im.cpu().numpy(), pos, 31)
        assert o.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(st.cpu().numpy(), want[2])
        nbytes = n * sh * sw * np.dtype(dt).itemsize
        out[f"extract_stamps_{name}"] = {"n": n, "ms": ms, "ms_all": allms, "bytes_out": nbytes,
                                         "GB_per_s_out": nbytes / ms / 1e6}
    # the yardstick: as many float64 bytes through bsgp_extract_tiles, boxes = the full stamps' boxes
    full = want[1][want[2] == 0]
    bx = torch.from_numpy(np.ascontiguousarray(np.resize(full, (n, 4)))).cuda()
    im = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float64)).cuda()
    o = torch.empty((n, sh, sw), dtype=torch.float64, device="cuda")

    def tiles():
        B.check(B.lib().bsgp_extract_tiles(B._ptr(im), H, W, B._ptr(bx), n, sh, sw, B._ptr(o),
                                           B.current_stream()))
    ms, allms = timed(tiles, launches)
    out["extract_tiles_f64_same_bytes"] = {"n": n, "ms": ms, "ms_all": allms,
                                           "bytes_out": n * sh * sw * 8,
                                           "GB_per_s_out": n * sh * sw * 8 / ms / 1e6}
    # the choice: n stars x 5 candidates of synthetic catalogue rows
    K, rng = 5, np.random.default_rng(1)
    res = rng.uniform(1.0, 3.0, (n * K, 1, 8))
    obs = rng.uniform(1.0, 3.0, (n, 1, 8))
    res[..., 6], obs[..., 6] = 0.3, 0.2
    nl = (rng.uniform(size=n * K) < 0.9).astype(np.int32)
    it = rng.integers(1, 500, n * K).astype(np.int32)
    dev = [torch.from_numpy(a).cuda() for a in (nl, res, obs, it)]

    def select():
        S._select_dev(*dev, n, K)
    ms, allms = timed(select, launches)
    got = [t.cpu().numpy() for t in S._select_dev(*dev, n, K)]
    want = ref.select_ref(nl, res, obs, it, K)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    out["stamp_select_with_output_allocation"] = {"n": n, "K": K, "ms": ms, "ms_all": allms}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--maxit", type=int, default=500)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    B.require_gpu()
    gold = os.path.join(ROOT, "tests", "golden")
    _, img = fits_io.read_fits(os.path.join(gold, "SUBDIV_ORIGIMG.fits"))
    _, psf = fits_io.read_fits(os.path.join(gold, "psfccfbrd210048_1_1_img.fits"))
    img = np.asarray(img, dtype=np.float32)
    pos = positions(img, a.n)
    r = {"device": torch.cuda.get_device_name(0), "frame": list(img.shape),
         "kernels": kernels(img, pos, a.launches),
         "kernels_65536_positions": kernels(img, positions(img, 65536, seed=1), 10),
         "driver": driver(img, np.asarray(psf), pos, a.reps, a.maxit)}
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
