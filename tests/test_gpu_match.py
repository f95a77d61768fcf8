"""The catalogue cross-match on the device (bsgp_match_catalogs)
against the numpy restatement tests/match_ref.py and the reference's four
published cross-matched tables (tests/golden/match_cases.npz): match1, match2,
npairs and status equal, sep1 bit for bit, on both paths."""
import os

import numpy as np
import pytest

import match_ref as ref
from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu
AUTO, LDS, GLOBAL = 0, 1, 2
PUBLISHED = ("subdiv", "subdiv_beta", "crowded", "crowded_beta")


@pytest.fixture(scope="module")
def sg():
    import segmentation
    return segmentation


@pytest.fixture(scope="module")
def fx():
    return golden("match_cases.npz")


def cats(fx, tag):
    return tuple({nm: fx[f"{tag}_cat{k}_{nm}"] for nm in ref.CAT_COLUMNS} for k in (1, 2))


def synthetic_case(fx, tag):
    kw = {k: fx[f"{tag}_{k}"] for k in ("valid1", "valid2") if f"{tag}_{k}" in fx}
    kw.update({k: int(fx[f"{tag}_{k}"]) for k in ("n1", "n2") if f"{tag}_{k}" in fx})
    return tuple(fx[f"{tag}_{k}"] for k in ("x1", "y1", "x2", "y2")), kw


def dev_match(images, max_sep, path=AUTO, cap1=None, cap2=None, rc=0):
    """One call of the entry point for a batch.  images: (x1, y1, x2, y2, kw)
    per image, kw holding n1 / n2 / valid1 / valid2 (n defaults to the arrays'
    length).  The rows from an image's length to the cap hold a copy of the
    other catalogue's first point, which a kernel that read them would match.
    Returns M5's outputs per image, cut to the arrays' length after checking
    that the rest is -1 / NaN."""
    import torch

    import _bsgp
    B = len(images)
    caps = [cap1 or max(1, max(len(im[0]) for im in images)),
            cap2 or max(1, max(len(im[2]) for im in images))]
    xy = [np.zeros((2, B, caps[0])), np.zeros((2, B, caps[1]))]
    n = np.zeros((2, B), np.int32)
    given = [any(f"valid{s + 1}" in im[4] for im in images) for s in (0, 1)]
    valid = [np.ones((B, caps[s]), np.int32) for s in (0, 1)]
    for b, im in enumerate(images):
        for s in (0, 1):
            x, y, ox, oy = im[2 * s], im[2 * s + 1], im[2 - 2 * s], im[3 - 2 * s]
            k = len(x)
            xy[s][0, b, :k], xy[s][1, b, :k] = x, y
            if len(ox) and np.isfinite(ox[0]) and np.isfinite(oy[0]):
                xy[s][0, b, k:], xy[s][1, b, k:] = ox[0], oy[0]
            n[s, b] = im[4].get(f"n{s + 1}", k)
            if f"valid{s + 1}" in im[4]:
                valid[s][b, :k] = im[4][f"valid{s + 1}"]
    dev = [torch.from_numpy(a).cuda() for a in xy]
    nd = torch.from_numpy(n).cuda()
    vd = [torch.from_numpy(valid[s]).cuda() if given[s] else None for s in (0, 1)]
    m1 = torch.full((B, caps[0]), 7, dtype=torch.int32, device="cuda")
    m2 = torch.full((B, caps[1]), 7, dtype=torch.int32, device="cuda")
    sp = torch.full((B, caps[0]), 7.0, dtype=torch.float64, device="cuda")
    npairs = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    side = [(_bsgp._ptr(dev[s][0]), _bsgp._ptr(dev[s][1]), 1, _bsgp._ptr(vd[s]), 1, caps[s],
             _bsgp._ptr(nd[s])) for s in (0, 1)]
    got = _bsgp.lib().bsgp_match_catalogs(*side[0], *side[1], B, float(max_sep), path,
                                          _bsgp._ptr(m1), _bsgp._ptr(m2), _bsgp._ptr(sp),
                                          _bsgp._ptr(npairs), _bsgp._ptr(st),
                                          _bsgp.current_stream())
    assert got == rc, (got, _bsgp.lib().bsgp_last_error())
    if rc:
        return None
    m1, m2, sp, npairs, st = (t.cpu().numpy() for t in (m1, m2, sp, npairs, st))
    out = []
    for b, im in enumerate(images):
        k1, k2 = len(im[0]), len(im[2])
        assert (m1[b, k1:] == -1).all() and (m2[b, k2:] == -1).all() and np.isnan(sp[b, k1:]).all()
        out.append(dict(match1=m1[b, :k1], match2=m2[b, :k2], sep1=sp[b, :k1],
                        npairs=int(npairs[b]), status=int(st[b])))
    return out


def same(got, want, what=""):
    for k in ("match1", "match2", "npairs", "status"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["sep1"].tobytes() == np.asarray(want["sep1"]).tobytes(), (what, "sep1")


def both_paths(image, max_sep, want, what=""):
    for path in (AUTO, LDS, GLOBAL):
        same(dev_match([image], max_sep, path)[0], want, (what, path))


@pytest.mark.parametrize("tag", PUBLISHED)
def test_published_table_on_the_device(sg, fx, tag):
    rest, orig = cats(fx, tag)
    m = sg.match_catalogs(rest, orig)  # the defaults: max_sep 1.1, catalogue 1 the restored one
    assert np.array_equal(m.labels1, fx[f"{tag}_pub_label_1"])
    assert np.array_equal(m.labels2, fx[f"{tag}_pub_label_2"])
    pub = fx[f"{tag}_pub_Separation"]
    assert np.max(np.abs(m.separation - pub) / pub) <= 1e-11
    assert m.status == 0 and m.n_pairs == len(pub) and not m.batched
    want = ref.match_greedy(rest["xcentroid"], rest["ycentroid"], orig["xcentroid"],
                            orig["ycentroid"], 1.1)
    same(dict(match1=m.match1, match2=m.match2, sep1=m.sep1, npairs=m.n_pairs, status=m.status), want)
    joined = sg.matched_columns(m, rest, orig)
    for nm in ref.CAT_COLUMNS:
        for k in ("_1", "_2"):
            assert np.array_equal(joined[nm + k], fx[f"{tag}_pub_{nm}{k}"]), nm + k
    # the per-star numbers the application's commented-out lines were after
    got = sg.matched_metrics(orig, rest)
    f1, f2 = fx[f"{tag}_pub_segment_flux_1"], fx[f"{tag}_pub_segment_flux_2"]
    assert np.array_equal(got["flux_fractional_difference"], 1 - f1 / f2)
    assert np.array_equal(got["fwhm_ratio"], fx[f"{tag}_pub_fwhm_1"] / fx[f"{tag}_pub_fwhm_2"])
    assert np.array_equal(got["orig_label"], fx[f"{tag}_pub_label_2"])
    assert got["n_pairs"] == len(pub)


@pytest.mark.parametrize("tag", PUBLISHED)
def test_published_catalogues_at_wider_radii(fx, tag):
    """Real conflicts: 2 to 5 accepting rounds."""
    c1, c2 = cats(fx, tag)
    xy = (c1["xcentroid"], c1["ycentroid"], c2["xcentroid"], c2["ycentroid"])
    rounds = []
    for r in (1.1, 2.0, 3.0, 5.0, 10.0, 40.0):
        want = ref.match_rounds(*xy, r)
        rounds.append(want["rounds"])
        both_paths(xy + ({},), r, want, r)
    assert max(rounds) >= 2, rounds


def test_synthetic_cases(fx):
    """Empty catalogues, 1 x 1 inside and outside, the inclusive bound, ties on
    a lattice and duplicated points, valid masks, NaN / inf coordinates, n
    above and below the cap: each against the fixture, on both paths."""
    for tag in fx["tags"]:
        xy, kw = synthetic_case(fx, tag)
        want = {k: fx[f"{tag}_{k}"] for k in ("match1", "match2", "sep1", "npairs", "status")}
        both_paths(xy + (kw,), float(fx[f"{tag}_max_sep"]), want, tag)
    assert fx["bound_in_npairs"] == 1 and fx["bound_out_npairs"] == 0
    assert fx["masked_status"] == ref.NONFINITE and fx["over_cap_status"] == ref.OVER_CAP


def test_chain_needs_forty_rounds(fx, monkeypatch):
    """The orphan-rescan logic's case: every round takes the last pair of the
    chain and orphans the row that had picked its partner.  Also the launch
    shape: one wave and sixteen waves give the same result."""
    x1, y1, x2, y2 = ref.chain(40)
    want = ref.match_rounds(x1, y1, x2, y2, 2.0)
    assert want["rounds"] == 40 and want["accepted"] == [1] * 40
    both_paths((x1, y1, x2, y2, {}), 2.0, want)
    for block in ("64", "1024"):
        monkeypatch.setenv("BSGP_MATCH_BLOCK", block)
        both_paths((x1, y1, x2, y2, {}), 2.0, want, block)
    # and with the catalogues exchanged
    want = ref.match_rounds(x2, y2, x1, y1, 2.0)
    assert want["rounds"] == 40
    both_paths((x2, y2, x1, y1, {}), 2.0, want)


def test_batch_gives_every_image_its_solo_result(fx):
    images = [synthetic_case(fx, f"batch{k}") for k in range(6)]
    images = [xy + (kw,) for xy, kw in images]
    assert sorted(len(im[0]) for im in images) == [0, 1, 64, 129, 255, 300]
    for path in (AUTO, GLOBAL):
        batch = dev_match(images, 1.5, path, cap1=320, cap2=333)  # caps above every n
        for k, im in enumerate(images):
            same(batch[k], dev_match([im], 1.5, path)[0], (k, "solo"))
            same(batch[k], {q: fx[f"batch{k}_{q}"] for q in ("match1", "match2", "sep1", "npairs",
                                                              "status")}, (k, "fixture"))


def uniform(seed, n1, n2, field):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, field, n1), rng.uniform(0, field, n1), rng.uniform(0, field, n2),
            rng.uniform(0, field, n2), {})


@pytest.mark.parametrize("n1,n2", ((2048, 2048), (2048, 2049)))
def test_path_boundary(n1, n2, monkeypatch):
    """n1 + n2 = 4096 is the LDS path's last size, 4097 the global path's first."""
    im = uniform(n1 + n2, n1, n2, 64.0)  # a point per unit area: conflicts at 1.5
    want = ref.match_rounds(*im[:4], 1.5)
    assert want["rounds"] >= 3 and want["npairs"] > 500
    same(dev_match([im], 1.5, AUTO)[0], want, "auto")
    same(dev_match([im], 1.5, GLOBAL)[0], want, "global")
    if n1 + n2 <= 4096:
        same(dev_match([im], 1.5, LDS)[0], want, "lds")
        monkeypatch.setenv("BSGP_MATCH_BLOCK", "192")  # another launch shape: 22 rows per lane
        same(dev_match([im], 1.5, LDS)[0], want, "lds, 192 threads")
    else:
        import _bsgp
        dev_match([im], 1.5, LDS, rc=_bsgp.BSGP_ERR_UNSUPPORTED)


def test_global_path_5000_by_5000():
    im = uniform(5000, 5000, 5000, 100.0)
    want = ref.match_rounds(*im[:4], 1.5)
    assert want["rounds"] >= 3 and want["npairs"] > 1000
    same(dev_match([im], 1.5, AUTO)[0], want)


def test_device_catalogues(sg):
    """Two batched device catalogues matched from their device columns: equal
    to the match of their host columns and to the restatement; a catalogue
    against itself matches every valid row to itself at separation 0."""
    import fits_io
    _, img = fits_io.read_fits(os.path.join(GOLDEN, "SUBDIV_ORIGIMG.fits"))
    img = np.asarray(img, dtype=np.float64)
    a, _ = sg.source_info(np.stack([img, img[::-1].copy()]), 60, device_out=True)
    b, _ = sg.source_info(np.stack([np.roll(img, 1, axis=1), 1.5 * img[::-1]]), 60, device_out=True)
    assert a.batched and hasattr(a, "f64_cols") and min(a.nlabels) > 50
    m = sg.match_catalogs(a, b, max_sep=2.0, device_out=True)
    host = [[dict(xcentroid=c["xcentroid"][k], ycentroid=c["ycentroid"][k], area=c["area"][k],
                  label=c["label"][k]) for k in (0, 1)] for c in (a, b)]
    h = sg.match_catalogs(host[0], host[1], max_sep=2.0)
    assert m.batched and h.batched and m.n_pairs.tolist() == h.n_pairs.tolist()
    for k in (0, 1):
        want = ref.match_greedy(a["xcentroid"][k], a["ycentroid"][k], b["xcentroid"][k],
                                b["ycentroid"][k], 2.0, valid1=a["area"][k], valid2=b["area"][k])
        for res in (m, h):
            same(dict(match1=res.match1[k], match2=res.match2[k], sep1=res.sep1[k],
                      npairs=res.n_pairs[k], status=res.status[k]), want, k)
        assert np.array_equal(m.labels1[k], m.idx1[k] + 1) and np.array_equal(m.labels2[k], m.idx2[k] + 1)
        assert m.n_pairs[k] > 40
    assert tuple(m.match1_dev.shape) == (2, max(a.nlabels)) and m.sep1_dev.is_cuda
    assert m.n_pairs_dev.cpu().tolist() == m.n_pairs.tolist()
    # unbatched device catalogues through the host functions
    one, _ = sg.source_info(img, 60, device_out=True)
    two, _ = sg.source_info(np.roll(img, 1, axis=1), 60, device_out=True)
    mm = sg.match_catalogs(two, one, max_sep=2.0)
    stars = sg.matched_metrics(one, two, max_sep=2.0)
    assert not mm.batched and stars["n_pairs"] == mm.n_pairs > 40
    assert (stars["n_orig"], stars["n_restored"]) == (one.nlabels, two.nlabels)
    assert np.array_equal(stars["fwhm_ratio"], two["fwhm"][mm.idx1] / one["fwhm"][mm.idx2])
    assert np.array_equal(stars["flux_fractional_difference"],
                          1 - two["segment_flux"][mm.idx1] / one["segment_flux"][mm.idx2])
    assert np.array_equal(stars["orig_label"], mm.idx2 + 1)
    table = sg.matched_columns(mm, two, one)
    assert list(table)[0] == "label_1" and list(table)[-1] == "Separation" and len(table) == 2 * len(sg.COLUMNS) + 1
    assert np.array_equal(table["xcentroid_2"], one["xcentroid"][mm.idx2])
    assert np.array_equal(table["Separation"], mm.separation)
    assert abs(np.median(mm.separation) - 1) < 0.01  # the shift (but for sources on the wrapped edge)
    me = sg.match_catalogs(a, a)
    for k in (0, 1):
        ok = a["area"][k] > 0
        assert np.array_equal(me.match1[k], np.where(ok, np.arange(len(ok)), -1))
        assert np.array_equal(me.match2[k], me.match1[k]) and (me.sep1[k][ok] == 0).all()
        assert np.isnan(me.sep1[k][~ok]).all() and me.n_pairs[k] == ok.sum()


def test_python_layer(sg, fx):
    rest, orig = cats(fx, "subdiv")
    xy1, xy2 = (rest["xcentroid"], rest["ycentroid"]), (orig["xcentroid"], orig["ycentroid"])
    base = sg.match_catalogs(rest, orig)
    for path in ("auto", "lds", "global"):
        m = sg.match_catalogs(xy1, xy2, path=path)  # (x, y) tuples carry no labels
        assert np.array_equal(m.match1, base.match1) and m.labels1 is None
        assert m.separation.tobytes() == base.separation.tobytes()
    mb = sg.match_catalogs([rest, xy2, ([], [])], [orig, xy1, xy1])
    assert mb.batched and mb.n_pairs.tolist() == [62, 62, 0]
    assert np.array_equal(mb.match1[0], base.match1) and np.array_equal(mb.match1[1], base.match2)
    assert len(mb.match1[2]) == 0 and len(mb.unmatched2[2]) == len(xy1[0])
    big = (np.zeros(2049), np.zeros(2049))
    with pytest.raises(ValueError, match="4096"):
        sg.match_catalogs(big, (np.zeros(2048), np.zeros(2048)), path="lds")


def test_every_error_return():
    import _bsgp
    ref.check_abi_errors(_bsgp)
