"""Time bsgp_background2d on the device: HIP events around the
C-ABI call with preallocated outputs, 2 warm-ups, median of 7.

Two workloads: one 2048x2048 field with box 64, and 1024 images of 256x256
with box 32 (float32 input, filter 3, defaults otherwise).  Each is put beside
a device-to-device copy of the bytes the call writes (same process) and
beside a numpy / scipy restatement on the host.  Variants of the call split
the time without a profiler: no maps (box statistics + mesh only: the zoom is
the rest), and maxiters=0 (sort and one pass of statistics: the clipping
iterations are the rest).

    python tools/bkg_timing.py --out profiles/bkg/timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "beta-sgp_amd"))

import _bsgp as B  # noqa: E402

torch = B.torch


def field(rng, shape):
    """Sky 100 + gradient, Poisson noise, a few hundred bright pixels per image."""
    n, H, W = shape
    yy, xx = np.mgrid[:H, :W]
    base = 100.0 + 20.0 * yy / H + 10.0 * xx / W
    d = rng.poisson(base[None].repeat(n, 0)).astype(np.float32)
    k = max(1, H * W // 2000)
    for i in range(n):
        d[i, rng.integers(0, H, k), rng.integers(0, W, k)] += rng.pareto(1.5, k).astype(np.float32) * 500
    return d


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


def host_restatement(d, box, sigma=3.0, maxiters=10):
    """numpy sigma clipping of every box at once + scipy filter / zoom per image."""
    from scipy import ndimage
    n, H, W = d.shape
    ny, nx = H // box, W // box
    out = np.empty((n, H, W))
    for i in range(n):
        v = d[i].astype(np.float64).reshape(ny, box, nx, box).swapaxes(1, 2).reshape(ny * nx, -1)
        for _ in range(maxiters):
            c, s = np.nanmedian(v, axis=1), np.nanstd(v, axis=1)
            bad = (v < (c - sigma * s)[:, None]) | (v > (c + sigma * s)[:, None])
            if not bad.any():
                break
            v = np.where(bad, np.nan, v)
        maps = []
        for m in (np.nanmedian(v, axis=1), np.nanstd(v, axis=1)):
            f = ndimage.generic_filter(m.reshape(ny, nx), np.nanmedian, size=3, mode="constant",
                                       cval=np.nan)
            z = ndimage.zoom(f, box, order=3, mode="reflect", grid_mode=True)
            maps.append(np.clip(z, f.min(), f.max()))
        out[i] = maps[0]  # the rms map is computed for the time only
    return out


def run(name, shape, box, host_images, rng):
    n, H, W = shape
    d = torch.from_numpy(field(rng, shape)).cuda()
    ny, nx = H // box, W // box
    f64 = dict(dtype=torch.float64, device="cuda")
    bkg, rms = torch.empty(shape, **f64), torch.empty(shape, **f64)
    mesh, rmesh = torch.empty((n, ny, nx), **f64), torch.empty((n, ny, nx), **f64)
    med = torch.empty((n, 2), **f64)
    st = torch.empty((n, 1 + 3 * ny * nx), dtype=torch.int32, device="cuda")

    def call(maps=True, maxiters=10):
        B.check(B.lib().bsgp_background2d(
            B._ptr(d), B.BSGP_DTYPE_F32, n, H, W, box, box, 3, 3, 3.0, maxiters, 10.0, 1, None,
            B._ptr(bkg) if maps else None, B._ptr(rms) if maps else None, B._ptr(mesh),
            B._ptr(rmesh), B._ptr(med), B._ptr(st), B.current_stream()))

    full, full_all = timed(call)
    iters = st.cpu().numpy()[:, 1 + 2 * ny * nx:]
    nomap, _ = timed(lambda: call(maps=False))
    nomap0, _ = timed(lambda: call(maps=False, maxiters=0))
    out_bytes = sum(t.numel() * t.element_size() for t in (bkg, rms, mesh, rmesh, med, st))
    src = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy, _ = timed(lambda: dst.copy_(src))
    sub = d[:host_images].cpu().numpy()
    t0 = time.perf_counter()
    ref = host_restatement(sub, box)
    host_s = time.perf_counter() - t0
    err = float(np.max(np.abs(bkg[:host_images].cpu().numpy() - ref)) / np.max(np.abs(ref)))
    r = {
        "workload": name, "images": n, "H": H, "W": W, "box": box, "input": "float32",
        "ms_call_median_of_7": full, "ms_call_all": full_all,
        "ms_without_maps": nomap, "ms_zoom_by_difference": full - nomap,
        "ms_without_maps_maxiters0": nomap0, "ms_clipping_iterations_by_difference": nomap - nomap0,
        "mean_clipping_iterations": float(iters.mean()), "max_clipping_iterations": int(iters.max()),
        "bytes_written": out_bytes, "bytes_read": int(d.numel() * 4),
        "ms_d2d_copy_of_bytes_written": copy,
        "GBps_written_by_call": out_bytes / full / 1e6,
        "GBps_written_by_zoom": 2 * n * H * W * 8 / max(full - nomap, 1e-9) / 1e6,
        "GBps_d2d_copy_written_side": out_bytes / copy / 1e6,
        "host_numpy_scipy_s": host_s, "host_images": host_images,
        "host_s_scaled_to_all_images": host_s * n / host_images,
        "device_vs_host_restatement_max_rel": err,
    }
    print(json.dumps(r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B.require_gpu()
    rng = np.random.default_rng(0)
    res = [run("field 2048^2, box 64", (1, 2048, 2048), 64, 1, rng),
           run("1024 x 256^2, box 32", (1024, 256, 256), 32, 32, rng)]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
