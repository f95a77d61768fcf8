"""Generate tests/golden/ref_rowwide_<case>.npz: this project's OWN outputs
at the commit before the per-wave row passes went to two-pixel (16-byte)
operand accesses, for tests/test_gpu_rowwide.py, which holds every later
build to them bit for bit.

Run on an MI355X at the commit whose bits are to be pinned (the library built
by __graft_entry__.build()):

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rowwide.py

Every case is beta-SGP with beta = 1.05, linear A, a 9x9 Gaussian PSF, stop
rule 1 and a scalar background of 100, on a batch of synthetic star fields
made by `field` below (not stored: the fixture keeps a SHA-256 of the batch,
so a numpy whose generator changes is noticed; the PSF is stored, numpy's
exp not being the same on every CPU).  Each case is solved four
ways, persistent 0 / 1 x float64 / float32 storage.  Stored per way: discr,
iters, flags and a SHA-256 of x; x itself for the float64 phase-kernel solve
(persistent 0) of the small cases, which keeps the files small and lets a
failure be looked at.
"""
import hashlib
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# name: (H, W, images, MAXIT, team)
CASES = {
    "64x64": (64, 64, 6, 8, 1),      # one full 64-column chunk
    "33x64": (33, 64, 6, 8, 1),      # odd H: the last row has no partner
    "40x70": (40, 70, 6, 8, 1),      # even W, partial second chunk, clamped pairs
    "48x130": (48, 130, 6, 8, 1),    # a chunk holding a single pair
    "31x31": (31, 31, 6, 8, 1),      # odd W: the one-pixel path
    "256x256": (256, 256, 2, 5, 1),
    "256x256_team8": (256, 256, 1, 3, 8),
}
WAYS = [(p, s) for s in ("f64", "f32") for p in (0, 1)]
KW = dict(init_recon=2, proj_type=1, stop_criterion=1, alpha=10.0, ccd_sat_level=65000.0,
          use_original_SGP_Afunction=False, schedule_lr=True, adapt_beta=False, betaParams=1.05)


def gaussian_psf(k=9, fwhm=2.25):
    sig = fwhm / 2.354820045030949
    c = (k - 1) / 2.0
    yy, xx = np.mgrid[0:k, 0:k]
    p = np.exp(-((yy - c) ** 2 + (xx - c) ** 2) / (2 * sig * sig))
    return p / p.sum()


def field(h, w, n, seed):
    """n images [n, h, w]: Moffat-like stars on a background of 100 plus
    uniform noise.  Only Generator.random(), + - * / and sqrt (all correctly
    rounded) enter, so every numpy and CPU makes the same bits; no exp."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w))
    for i in range(n):
        img = np.full((h, w), 100.0)
        for _ in range(max(4, h * w // 256)):
            cy, cx, a, s = rng.random(4)
            q = 1.0 + ((yy - cy * h) * (yy - cy * h) + (xx - cx * w) * (xx - cx * w)) / (
                (1.5 + 2.5 * s) * (1.5 + 2.5 * s))
            img += (200.0 + 3000.0 * a * a) / (q * q * q)
        out[i] = img + np.sqrt(img) * (2.0 * rng.random((h, w)) - 1.0)
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def inputs(name):
    h, w, n, maxit, team = CASES[name]
    gns = field(h, w, n, seed=1000 + h * 7 + w)
    return gns, dict(KW, MAXIT=maxit, team=team)


def solve(sgp, name, psf, persistent, storage):
    gns, kw = inputs(name)
    return sgp.sgp_betaDiv_batch(gns, psf, 100.0, persistent=persistent, storage=storage, **kw)


def main():
    for p in (ROOT, os.path.join(ROOT, "beta-sgp_amd")):
        sys.path.insert(0, p)
    import _bsgp
    _bsgp.require_gpu()
    import sgp
    for name in CASES:
        gns, _ = inputs(name)
        psf = gaussian_psf()
        out = dict(gn_sha=np.array(sha(gns)), psf=psf)
        for persistent, storage in WAYS:
            r = solve(sgp, name, psf, persistent, storage)
            k = f"p{persistent}_{storage}_"
            out[k + "x_sha"] = np.array(sha(r["x"]))
            out[k + "discr"], out[k + "iters"] = r["discr"], r["iters"]
            out[k + "flags"] = r["flags"]
            if persistent == 0 and storage == "f64" and gns[0].size <= 64 * 130:
                out[k + "x"] = r["x"]
        path = os.path.join(HERE, f"ref_rowwide_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
