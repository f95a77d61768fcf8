"""Time the background-matched co-add on the device
against the plain co-add: HIP events, 3 warm-ups, median of 11 launches.

Two fields, tiles cut from a smooth field plus a constant per tile plus noise
(so every overlap has its own median):
  * 81 tiles of 256 x 256 at overlap 32 on 2048 x 2048 (272 pairs);
  * 25 tiles of 375 x 375, the application's subdivision size, at overlap 37
    on 1727 x 1727 (72 pairs).
Timed: coadd_tiles as it is without matching; coadd_tiles(match_background=
True) as a whole, for a layout seen before and for a new one (the pair search
on the host and its upload included); its three device
steps one call each with preallocated outputs (bsgp_tile_offsets,
bsgp_tile_corrections, bsgp_coadd_tiles_matched); tile_pairs on the host; the
numpy restatement tests/coadd_ref.py on the host.  Also recorded: the
conjugate gradients' iterations and the relative residual they reached, and
the corrections' distance from numpy's lstsq.

    python tools/coadd_timing.py --out profiles/coadd/timing.json
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
import coadd_ref  # noqa: E402
import subdivisions as S  # noqa: E402

torch = B.torch


def timed(fn, warm=3, reps=11):
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


def one(shape, tile, overlap, host_ref):
    rng = np.random.default_rng(shape[0])
    boxes = S.subdivision_boxes(shape, tile, overlap)
    n = len(boxes)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    field = 50 + 0.01 * xx + 0.005 * yy + 3 * np.sin(xx / 90.0) * np.cos(yy / 70.0)
    t = np.stack([field[y0:y1, x0:x1] for x0, y0, x1, y1 in boxes])
    t = t + rng.normal(0, 5, n)[:, None, None] + rng.normal(0, 0.3, t.shape)
    td = B.to_dev(t)
    H, W = shape
    r = {"field": list(shape), "tile": list(tile), "overlap": overlap, "tiles": n}
    t0 = time.perf_counter()
    g = S.tile_pairs(boxes)
    r["ms_host_tile_pairs"] = (time.perf_counter() - t0) * 1e3
    r["pairs"] = len(g.pairs)
    r["ms_coadd_plain"], r["ms_coadd_plain_all"] = timed(lambda: S.coadd_tiles(td, boxes, shape))
    r["ms_coadd_match_background"], r["ms_coadd_match_background_all"] = timed(
        lambda: S.coadd_tiles(td, boxes, shape, match_background=True))

    def new_layout():  # the pair search and its upload every call
        S._geometry.clear()
        return S.coadd_tiles(td, boxes, shape, match_background=True)

    r["ms_coadd_match_background_new_layout"], _ = timed(new_layout)
    # the three device steps, one call each
    m, bd = S._match_dev(td, boxes, None)
    _, geo, sizes = S._geometry_dev(boxes)
    _, prd, row_ptr, nbr, nbr_pair, nbr_sign, comp = torch.split(geo, sizes)
    L, s = B.lib(), B.current_stream
    th, tw = tile
    P = len(g.pairs)
    mean = torch.empty(shape, dtype=torch.float64, device="cuda")
    foot = torch.empty_like(mean)
    off, corr, st, info = m.offsets, m.corrections, m.status, m.solve_info
    r["ms_tile_offsets"], _ = timed(lambda: B.check(L.bsgp_tile_offsets(
        B._ptr(td), n, th, tw, B._ptr(bd), B._ptr(prd), P, B._ptr(off), B._ptr(st), s())))
    r["ms_tile_corrections"], _ = timed(lambda: B.check(L.bsgp_tile_corrections(
        n, B._ptr(row_ptr), B._ptr(nbr), B._ptr(nbr_pair), B._ptr(nbr_sign), B._ptr(comp), g.ncomp,
        B._ptr(off), -1, B._ptr(corr), B._ptr(st), B._ptr(info), s())))
    r["ms_coadd_tiles_matched"], _ = timed(lambda: B.check(L.bsgp_coadd_tiles_matched(
        B._ptr(td), n, th, tw, B._ptr(bd), B._ptr(corr), H, W, B._ptr(mean), B._ptr(foot), s())))
    h = m.to_host(warn=False)
    r["cg_iterations"], r["cg_relative_residual"] = int(h.solve_info[0]), float(h.solve_info[1])
    r["status_or"] = int(np.bitwise_or.reduce(h.status))
    c, _ = coadd_ref.corrections(n, g.pairs, h.offsets)
    r["corrections_vs_lstsq_rel"] = float(np.abs(h.corrections - c).max() / np.abs(c).max())
    if host_ref:
        t0 = time.perf_counter()
        ref = coadd_ref.matched(t, boxes, shape)
        r["ms_host_coadd_ref"] = (time.perf_counter() - t0) * 1e3
        r["offsets_equal_numpy_median"] = bool(np.array_equal(ref[3], h.offsets))
        rm, _ = coadd_ref.coadd(t, boxes, shape, h.corrections)
        r["mosaic_equal_restatement"] = bool(np.array_equal(rm, mean.cpu().numpy()))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host-ref", action="store_true")
    a = ap.parse_args()
    B.require_gpu()
    r = {"device": torch.cuda.get_device_name(0),
         "fields": [one((2048, 2048), (256, 256), 32, not a.no_host_ref),
                    one((1727, 1727), (375, 375), 37, not a.no_host_ref)]}
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
