"""Time the catalogue cross-match (bsgp_match_catalogs) on the
device: HIP events, 2 warm-ups, median of 7, outputs preallocated.

Workloads: the crowded beta pair of the reference's published tables (407
restored x 392 original sources, tests/golden/match_cases.npz) alone and as a
batch of 30 (what follows the catalogues of 30 candidate tiles); 2048 x 2048
uniform random points in a 2048^2 field at max_sep 1.1 (the LDS path's largest
size; also on the global path); 16384 x 16384 in an 8192^2 field on the global
path.  Each is timed at every workgroup size of --blocks (the library's
BSGP_MATCH_BLOCK, read per call) and checked against the numpy restatement
tests/match_ref.py, which is timed next to it on the host and gives the
rounds.  The catalogue kernel bsgp_segment_catalog on the 30 tiles of
tools/localbkg_timing.py is timed in the same run, as the yardstick.

    python tools/match_timing.py --out profiles/match/timing.json
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
import match_ref as ref  # noqa: E402
import segmentation as S  # noqa: E402

torch = B.torch
PATHS = {"lds": B.BSGP_MATCH_LDS, "global": B.BSGP_MATCH_GLOBAL}


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


def workload(x1, y1, x2, y2, copies, max_sep, paths, blocks):
    """Times `copies` images of one pair; returns the figures and checks every
    image against the restatement."""
    t0 = time.perf_counter()
    want = ref.match_rounds(x1, y1, x2, y2, max_sep)
    host_ms = (time.perf_counter() - t0) * 1e3
    n1, n2 = len(x1), len(x2)
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    xy1 = torch.from_numpy(np.stack([x1, y1])).cuda()[:, None, :].repeat(1, copies, 1).contiguous()
    xy2 = torch.from_numpy(np.stack([x2, y2])).cuda()[:, None, :].repeat(1, copies, 1).contiguous()
    m1, m2 = torch.empty((copies, n1), **i32), torch.empty((copies, n2), **i32)
    sp, npairs, st = torch.empty((copies, n1), **f64), torch.empty((copies,), **i32), torch.empty((copies,), **i32)
    L, s = B.lib(), B.current_stream
    r = {"n1": n1, "n2": n2, "images": copies, "max_sep": max_sep, "pairs": int(want["npairs"]),
         "rounds": int(want["rounds"]), "accepted_per_round": want["accepted"],
         "ms_numpy_restatement_one_image": host_ms}
    for path in paths:
        def call():
            B.check(L.bsgp_match_catalogs(B._ptr(xy1[0]), B._ptr(xy1[1]), 1, None, 1, n1, None,
                                          B._ptr(xy2[0]), B._ptr(xy2[1]), 1, None, 1, n2, None, copies,
                                          max_sep, PATHS[path], B._ptr(m1), B._ptr(m2), B._ptr(sp),
                                          B._ptr(npairs), B._ptr(st), s()))
        for block in blocks:
            os.environ["BSGP_MATCH_BLOCK"] = str(block)
            t, allt = timed(call)
            for b in (0, copies - 1):
                assert np.array_equal(m1[b].cpu().numpy(), want["match1"])
                assert np.array_equal(m2[b].cpu().numpy(), want["match2"])
                assert sp[b].cpu().numpy().tobytes() == want["sep1"].tobytes()
            r[f"ms_{path}_block_{block}"], r[f"ms_{path}_block_{block}_all"] = t, allt
        del os.environ["BSGP_MATCH_BLOCK"]
        r[f"ms_{path}_default_block"] = timed(call)[0]
    return r


def catalogue_yardstick(images=30):
    """bsgp_segment_catalog on the 30 tiles of tools/localbkg_timing.py."""
    _, img = fits_io.read_fits(os.path.join(ROOT, "tests", "golden", "SUBDIV_ORIGIMG.fits"))
    tiles = np.stack([img * np.float32(1.0 + k / 100.0) for k in range(images)])
    H, W = img.shape
    cat, _ = S.source_info(tiles, 60, 5, deblend=True, device_out=True)
    cap = cat.int_cols.shape[1]
    nlab = torch.from_numpy(np.asarray(cat.nlabels, dtype=np.int32)).cuda()
    ic = torch.empty((images, cap, 5), dtype=torch.int32, device="cuda")
    fc = torch.empty((images, cap, 8), dtype=torch.float64, device="cuda")
    st = torch.empty((images,), dtype=torch.int32, device="cuda")
    sub, conv, lab = cat.data, cat.convolved_data, cat.segment_img.data

    def measure():
        B.check(B.lib().bsgp_segment_catalog(B._ptr(sub), B._ptr(conv), B._ptr(lab), images, H, W, cap,
                                             B._ptr(nlab), B._ptr(ic), B._ptr(fc), B._ptr(st),
                                             B.current_stream()))
    # and a match of such a batch through the Python layer, from the device columns
    t_match, _ = timed(lambda: S.match_catalogs(cat, cat))
    return {"images": images, "sources_total": int(np.sum(cat.nlabels)),
            "ms_segment_catalog": timed(measure)[0],
            "ms_match_catalogs_python_device_columns_self_match": t_match}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", default="64,128,256,512,1024")
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    blocks = [int(b) for b in a.blocks.split(",")]
    B.require_gpu()
    with np.load(os.path.join(ROOT, "tests", "golden", "match_cases.npz")) as z:
        cb = [z[f"crowded_beta_cat{k}_{c}centroid"] for k in (1, 2) for c in ("x", "y")]
    rng = np.random.default_rng(2048)
    u2048 = [rng.uniform(0, 2048.0, 2048) for _ in range(4)]
    d2048 = [rng.uniform(0, 45.0, 2048) for _ in range(4)]  # a point per unit area: conflicts
    r = {"device": torch.cuda.get_device_name(0), "blocks": blocks,
         "crowded_beta_alone": workload(*cb, 1, 1.1, ("lds", "global"), blocks),
         "crowded_beta_batch_30": workload(*cb, 30, 1.1, ("lds", "global"), blocks),
         "uniform_2048": workload(*u2048, 1, 1.1, ("lds", "global"), blocks),
         "dense_2048": workload(*d2048, 1, 1.5, ("lds", "global"), blocks),
         "catalogue_yardstick": catalogue_yardstick()}
    if not a.skip_large:
        u16k = [rng.uniform(0, 8192.0, 16384) for _ in range(4)]
        r["uniform_16384"] = workload(*u16k, 1, 1.1, ("global",), [b for b in blocks if b >= 256])
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
