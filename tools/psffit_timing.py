"""Time the PSF fit on the device: HIP events around the two
C-ABI calls (bsgp_psf_fit_moments, bsgp_psf_fit_solve) on inputs already on
the device (the outputs come from torch's caching allocator inside the timed
region, as fit_psf takes them), 2 warm-ups, median of 7.

Shapes: 100 stars with hw = 15 on a 450 x 450 frame (the reference's NPSF_MAX
and PSFHW on one of DIAPL's sub-frames), and a batch of 81 such frames; each
with niter = 0 and with niter = 3 (three of the stars carry a neighbour that
the clipping drops).  The numpy restatement of the estimator
(tests/psffit_ref.py) on the host, one frame, is put beside both.

    python tools/psffit_timing.py --out profiles/psffit/timing.json
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

SHAPES = [("frame", 1), ("batch_81", 81)]
HW, SIZE, NSTARS = 15, 450, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import _bsgp as B
    import psf_calculate as pc
    import psffit_ref as R
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

    cfg = R.config(HW, SIZE, SIZE)
    img, xy, flux, coef = R.make_frame(cfg, NSTARS, 1, sky=R.SKY, noise=1e-3)
    for k in (3, 30, 60):  # three stars with a neighbour, for the clipping rounds to drop
        R.add_star(img, cfg, coef, xy[k, 0] + 3.0, xy[k, 1], 0.3 * flux[k], at=tuple(xy[k]))
    res = {"shapes": {}}

    # the restatement on the host: one frame
    t0 = time.perf_counter()
    ref = R.fit(cfg, img, xy, flux=flux, sky=R.SKY)
    t_host = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    R.fit(cfg, img, xy, flux=flux, sky=R.SKY, niter=3, nsig=3.0)
    t_host3 = (time.perf_counter() - t0) * 1e3
    res["numpy_restatement_ms"] = {"niter0": t_host, "niter3": t_host3}
    print(f"numpy restatement, one frame: {t_host:.1f} ms (niter 0), {t_host3:.1f} ms (niter 3)")

    for name, nb in SHAPES:
        imgs = np.broadcast_to(img, (nb,) + img.shape).copy()
        pos = np.broadcast_to(xy, (nb,) + xy.shape).copy()
        fl = np.broadcast_to(flux, (nb,) + flux.shape).copy()
        fit = pc.fit_psf(imgs, pos, hw=HW, shape=cfg["shape"], flux=fl, background=R.SKY,
                         device_out=True)
        c, dev = dict(fit._cfg), dict(fit._dev)
        err = R.stamp_error(cfg, fit.coeffs[0].cpu().numpy(), ref["coef"], xy[:8])
        assert err < 1e-10, err
        row = {"B": nb, "stars": NSTARS, "hw": HW, "H": SIZE, "W": SIZE}
        row["moments_ms"], row["moments_all_ms"] = timed(lambda: pc._fit_moments_dev(c, dev, None))
        row["solve_ms"], row["solve_all_ms"] = timed(lambda: pc._fit_solve_dev(c, dev))
        c3 = dict(c, niter=3, nsig=3.0)
        row["solve_niter3_ms"], row["solve_niter3_all_ms"] = timed(lambda: pc._fit_solve_dev(c3, dev))
        row["rounds_niter3"] = int(dev["frame"][0, 1])
        t0 = time.perf_counter()
        pc.fit_psf(imgs, pos, hw=HW, shape=cfg["shape"], flux=fl, background=R.SKY)
        row["fit_psf_host_to_host_ms"] = (time.perf_counter() - t0) * 1e3  # with the copies to and from the device
        res["shapes"][name] = row
        print(name, json.dumps({k: (round(v, 4) if isinstance(v, float) else v)
                                for k, v in row.items() if not k.endswith("all_ms")}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
