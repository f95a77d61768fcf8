"""Writes tests/golden/starfind_cases.npz: the small frames of the star-finding
tests and what the numpy restatement tests/starfind_ref.py makes
of them.  Every frame is made here from a seed, stored as float32 (the float64
runs widen it); nothing comes from elsewhere.

As make_golden_localbkg.py does, the script asserts that no decision of a case
sits on its bound, so that the device's other summation order of a sky cannot
flip it: no correlation within 1e-9 of c_min, no significance within 1e-9
(relative) of thresh, no squared distance within 1e-9 of dxy^2, no sky value
within 1e-9 (relative) of a clipping bound and no |mean - median| / std within
1e-6 of 0.3.  A case that fails is changed, not tolerated.

    python tests/golden/make_golden_starfind.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import starfind_ref as ref  # noqa: E402

MARGIN_CORR = MARGIN_SIG = MARGIN_DXY = MARGIN_CLIP = 1e-9
MARGIN_BRANCH = 1e-6


def gauss(shape, x, y, amp, fwhm):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    s = fwhm * ref.FWHM_TO_SIGMA
    return amp * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))


def check_margins(res, kw, name):
    """No decision of a restatement result on its bound."""
    m = res["margins"]
    assert m["corr"] > MARGIN_CORR, (name, "corr", m)
    assert m["sig"] > MARGIN_SIG, (name, "significance", m)
    dxy2 = kw.get("dxy", 1.0) ** 2
    d2 = res["d2"][np.isfinite(res["d2"])]
    assert np.all(np.abs(d2 - dxy2) > MARGIN_DXY), (name, "dxy", d2)
    assert np.all(res["margin"] > MARGIN_CLIP), (name, "clip", res["margin"].min())
    assert np.all(res["branch"] > MARGIN_BRANCH), (name, "0.3 test", res["branch"].min())
    # a sky within its bar of the aperture flux's zero would flip BAD_FLUX
    n = res["template"]["n"]
    fin = np.isfinite(res["flux"])
    assert np.all(np.abs(res["flux"][fin]) > 1e3 * n * res["bar"][fin]), (name, "flux sign")


def scene():
    """40 x 56: an isolated star, a pair 3 px apart, a star whose peak is
    exactly R from the border and one at R - 1, a saturated plateau, a NaN
    inside one star's support and a masked pixel inside another's annulus."""
    rng = np.random.default_rng(20261021)
    shape, fwhm = (40, 56), 2.5  # rap = 3.0, R = 3
    img = 100.0 + 2.0 * rng.standard_normal(shape)
    for x, y, a in ((28, 20, 800.0), (10, 28, 600.0), (13, 28, 500.0), (3, 12, 700.0),
                    (45, 2, 700.0), (44, 30, 5000.0), (20, 33, 650.0)):
        img += gauss(shape, x, y, a, fwhm)
    sat = 3000.0
    img = np.minimum(img, sat).astype(np.float32)
    img[34, 21] = np.nan
    mask = np.zeros(shape, np.uint8)
    mask[20, 35] = 1  # 7 px from the isolated star: inside its annulus 6..9
    kw = dict(fwhm=fwhm, noise=2.0, sat_level=sat, anrad1=6.0, anrad2=9.0)
    return img, mask, kw


def sky_frames():
    """64 x 64 frames with a star at (32, 32) and one at (6, 6) (its annulus
    8..12 is cut by the corner): a constant sky (std 0: the mean), a symmetric
    one (2.5 median - 1.5 mean) and a bimodal one (|mean - median| / std above
    0.3: the median)."""
    rng = np.random.default_rng(7)
    shape = (64, 64)
    const = np.full(shape, 50.0)
    sym = 100.0 + 3.0 * rng.standard_normal(shape)
    hi = rng.random(shape) < 0.3
    skew = np.where(hi, 110.0, 100.0) + rng.standard_normal(shape)
    out = {}
    for name, f in (("const", const), ("sym", sym), ("skew", skew)):
        f = f + gauss(shape, 32, 32, 900.0, 3.0) + gauss(shape, 6, 6, 700.0, 3.0)
        out[name] = f.astype(np.float32)
    return out, dict(fwhm=3.0, noise=3.0, anrad1=8.0, anrad2=12.0)


def few_mask():
    """The mask that leaves 6 values of the annulus 8..12 about (32, 32)."""
    yy, xx = np.mgrid[:64, :64]
    d2 = (xx - 32) ** 2 + (yy - 32) ** 2
    ann = (d2 >= 64) & (d2 <= 144)
    m = ann.astype(np.uint8)
    ys, xs = np.nonzero(ann)
    m[ys[:6], xs[:6]] = 0
    return m


def lattice():
    """96 x 96: narrow stars every 6 px, amplitudes that differ."""
    rng = np.random.default_rng(11)
    shape = (96, 96)
    img = 20.0 + 0.5 * rng.standard_normal(shape)
    for y in range(4, 96, 6):
        for x in range(4, 96, 6):
            img += gauss(shape, x, y, 300.0 + 5.0 * ((x * 7 + y * 3) % 17), 1.7)
    return img.astype(np.float32), dict(fwhm=1.7, noise=0.5, anrad1=3.0, anrad2=5.5)


def batch():
    """3 x 48 x 48: two star fields around a constant frame, their noise levels
    and noise maps."""
    rng = np.random.default_rng(5)
    shape = (48, 48)
    frames, noise = [], [1.5, 1.0, 3.0]
    for b in range(3):
        if b == 1:
            frames.append(np.full(shape, 33.0))
            continue
        f = 60.0 + noise[b] * rng.standard_normal(shape)
        for _ in range(6):
            f += gauss(shape, rng.uniform(6, 42), rng.uniform(6, 42), rng.uniform(150, 900), 2.8)
        frames.append(f)
    nmap = np.stack([np.full(shape, n) * (1.0 + 0.2 * np.linspace(0, 1, 48))[None, :] for n in noise])
    return (np.stack(frames).astype(np.float32), np.array(noise), nmap.astype(np.float32),
            dict(fwhm=2.8, anrad1=7.0, anrad2=10.0))


def main():
    out = {}
    rng = np.random.default_rng(1)
    out["noise_frame"] = (1000.0 + 30.0 * rng.standard_normal((70, 150))).astype(np.float32)

    img, mask, kw = scene()
    res = ref.find_stars(img, mask=mask, **kw)
    check_margins(res, kw, "scene")
    peaks = set(zip(res["ic"].tolist(), res["ir"].tolist()))
    assert (28, 20) in peaks and (10, 28) in peaks and (13, 28) in peaks, peaks
    assert (3, 12) in peaks and not any(y < 3 for _, y in peaks), peaks
    assert (20, 33) not in peaks, "the NaN invalidates that peak pixel"
    k = int(np.flatnonzero((res["ic"] == 44) & (np.abs(res["ir"] - 30) <= 1))[0])
    assert res["nsat"][k] > 1, "the plateau holds several saturated pixels"
    out.update(scene_img=img, scene_mask=mask, scene_kw=repr(kw))
    for c in ref.FCOLS + ("ic", "ir", "nsat", "status"):
        out["scene_" + c] = res[c]
    print(f"scene: {len(res['ic'])} candidates, status {res['status'].tolist()}")

    frames, kw = sky_frames()
    for name, f in frames.items():
        for alg in ("mode", "median", "mean"):
            res = ref.find_stars(f, bkg_alg=alg, **kw)
            check_margins(res, kw, f"sky_{name}_{alg}")
        res = ref.find_stars(f, **kw)
        k = int(np.flatnonzero((res["ic"] == 32) & (res["ir"] == 32))[0])
        s = ref.sky(f, 32, 32, kw["anrad1"], kw["anrad2"])
        want = dict(const=np.inf, sym=None, skew=None)[name]
        if name == "const":
            assert s["branch"] == want and s["status"] == 0
        else:
            lo, hi, _, med, mean, sd, _ = ref.clip_sorted(ref.annulus_values(f, 32, 32, 8.0, 12.0))
            ratio = abs(mean - med) / sd
            assert (ratio < 0.3) == (name == "sym"), (name, ratio)
        assert any((res["ic"] == 6) & (res["ir"] == 6)), "the corner star is found"
        out["sky_" + name] = f
        out[f"sky_{name}_bkg"] = res["bkg"]
        print(f"sky {name}: bkg at (32, 32) {res['bkg'][k]!r}, {len(res['ic'])} candidates")
    out["sky_kw"] = repr(kw)
    fm = few_mask()
    res = ref.find_stars(frames["sym"], mask=fm, **kw)
    k = int(np.flatnonzero((res["ic"] == 32) & (res["ir"] == 32))[0])
    assert res["status"][k] & ref.FEW_SKY and np.isnan(res["bkg"][k]) and res["nsky"][k] == 6
    check_margins(res, kw, "few")
    out["sky_few_mask"] = fm

    img, kw = lattice()
    res = ref.find_stars(img, **kw)
    check_margins(res, kw, "lattice")
    assert len(res["ic"]) >= 200, len(res["ic"])  # several chunks of 2048 pixels hold some
    assert len(set((res["ir"] * 96 + res["ic"]) // 2048)) >= 4
    out.update(lattice_img=img, lattice_kw=repr(kw), lattice_n=len(res["ic"]))
    print(f"lattice: {len(res['ic'])} candidates")

    frames, noise, nmap, kw = batch()
    for b in range(3):
        for nz in (noise[b], nmap[b].astype(np.float64)):
            res = ref.find_stars(frames[b], noise=nz, **kw)
            check_margins(res, kw, f"batch{b}")
            assert (len(res["ic"]) == 0) == (b == 1)
    out.update(batch_img=frames, batch_noise=noise, batch_nmap=nmap, batch_kw=repr(kw))

    # the project's own frame with the parameters of the end-to-end test: margins only
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "beta-sgp_amd"))
    import fits_io
    _, img = fits_io.read_fits(os.path.join(HERE, "SUBDIV_ORIGIMG.fits"))
    kw = dict(fwhm=4.5, noise=9.8, thresh=3.0)
    res = ref.find_stars(np.asarray(img).astype(np.float32), **kw)
    check_margins(res, kw, "subdiv")
    print(f"SUBDIV_ORIGIMG: {len(res['ic'])} candidates, "
          f"{int(((res['status'] & ref.REJECTED) == 0).sum())} kept")

    np.savez_compressed(os.path.join(HERE, "starfind_cases.npz"), **out)
    print("wrote starfind_cases.npz,", os.path.getsize(os.path.join(HERE, "starfind_cases.npz")), "bytes")


if __name__ == "__main__":
    main()
