"""Save and resume of batched solves (include/bsgp.h bsgp_state_save /
bsgp_solve_resume, sgp.sgp_resume): a run split into segments is the unsplit
run bit for bit, on every path the solver has.  MI355X tests.

"Bitwise" is np.array_equal on x, iters, discr, crit, flags, beta_final and all
eight counters (`times` is wall time and exempt).  Every split saves its state,
then runs an unrelated solve on the same cached plan, and only then resumes:
the record alone carries the solve.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, crowded_case, golden, ref_kwargs, stamp_case

pytestmark = pytest.mark.gpu

SOLVE_RTOL = 1e-5  # the bar of test_gpu_parity.test_solve_matches_reference_linear
KEYS = ("x", "iters", "discr", "crit", "flags", "beta_final", "counters")


@pytest.fixture(scope="module")
def sgpmod():
    import _bsgp
    _bsgp.require_gpu()
    import sgp
    return sgp


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b))


def same(whole, part, rows=None):
    """`part` (a resumed solve) equals `whole` bit for bit; `rows` picks images
    of `whole`.  History arrays may differ in width (MAXIT + 1 of each call):
    the common columns are equal and the rest is the zero fill."""
    for k in KEYS:
        w, p = whole[k], part[k]
        if w is None and p is None:
            continue
        if rows is not None:
            w = w[rows]
        if k in ("discr", "crit", "flags") and w.shape[1] != p.shape[1]:
            n = min(w.shape[1], p.shape[1])
            assert not np.any(w[:, n:]) and not np.any(p[:, n:]), k
            w, p = w[:, :n], p[:, :n]
        np.testing.assert_array_equal(p, w, err_msg=k)


def solver(sgpmod, fn):
    return sgpmod.sgp_betaDiv_batch if fn == "sgp_betaDiv" else sgpmod.sgp_batch


def split_run(sgpmod, fn, gns, psf, bkg, cuts, MAXIT, kw, resume_kw=None, first_kw=None):
    """The solve in segments ending at `cuts` and MAXIT, with an unrelated solve
    on the same plan after every save.  Returns (last outputs, last state, every
    segment's outputs)."""
    run = solver(sgpmod, fn)
    kw = dict(kw)
    noise = dict(kw, MAXIT=3, **(first_kw or {}))
    junk = np.roll(np.asarray(gns), 3, axis=1)[:, ::-1].copy()
    out = run(gns, psf, bkg, MAXIT=cuts[0], return_state=True, **kw, **(first_kw or {}))
    segs = [out]
    for m in list(cuts[1:]) + [MAXIT]:
        st = out["state"]
        assert np.all(st.iters_done <= m)
        run(junk, psf, bkg, **noise)  # overwrites the plan's workspace
        out = sgpmod.sgp_resume(st, m, return_state=True, **(resume_kw or {}))
        segs.append(out)
    return out, out["state"], segs


def lin_case(name):
    fx = golden(f"ref_{name}.npz")
    kw = ref_kwargs(fx)
    if not np.isnan(fx["flux"]):
        kw["flux"] = np.float64(fx["flux"])
    bkg = fx["bkg"][None] if fx["bkg"].ndim else float(fx["bkg"])
    return fx, fx["gn"].astype(np.float64)[None], bkg, kw, str(fx["fn"])


# ------------------------------------------------- 1. phase kernels, split = whole
@pytest.mark.parametrize("case", ["beta", "adapt", "kl", "bmap", "f32storage", "xones"])
def test_phase_kernels_split_equals_whole(sgpmod, case):
    """MAXIT 12 whole, 5 + 7 and 5 + 3 + 4 (two resumes), persistent=0.  The
    runs with a fixture's own keywords are then continued to the fixture's
    MAXIT and meet its bar (SOLVE_RTOL, discr rtol 1e-7, iters)."""
    name = {"kl": "lin64_kl", "bmap": "lin64_beta_bmap"}.get(case, "lin64_beta")
    fx, gns, bkg, kw, fn = lin_case(name)
    maxit_fx = kw.pop("MAXIT")
    kw.update(stop_criterion=1, persistent=0, team=1)
    cuts2, cuts3 = [5], [5, 8]
    if case == "adapt":
        kw.update(adapt_beta=True, schedule_lr=True)
    elif case == "f32storage":
        kw.update(storage="f32")
    elif case == "xones":  # X = ones in iteration 1 only: the hand-over crosses it
        kw.update(init_recon=0)
        cuts2, cuts3 = [1], [1, 6]
    whole = solver(sgpmod, fn)(gns, fx["psf"], bkg, MAXIT=12, **kw)
    assert int(whole["iters"][0]) == 12
    two, _, _ = split_run(sgpmod, fn, gns, fx["psf"], bkg, cuts2, 12, kw)
    same(whole, two)
    three, st, segs = split_run(sgpmod, fn, gns, fx["psf"], bkg, cuts3, 12, kw)
    same(whole, three)
    # the counters are cumulative and the history rows complete in every segment
    assert np.all(np.diff([s["counters"][0, 1] for s in segs]) > 0)
    assert np.all(np.diff(three["times"][0, :13]) > 0)
    assert list(st.iters_done) == [12] and not st.stopped.any()
    if case in ("beta", "kl", "bmap"):
        end = sgpmod.sgp_resume(st, maxit_fx)
        it = int(end["iters"][0])
        assert it == int(fx["iters"])
        assert rel(end["x"][0], fx["x"]) < SOLVE_RTOL, rel(end["x"][0], fx["x"])
        np.testing.assert_allclose(end["discr"][0, :it + 1], fx["discr"], rtol=1e-7)


# ------------------------------------------------------------------ 2. odd size
@pytest.mark.parametrize("nimg", [1, 4])
def test_odd_size_stamps(sgpmod, nimg):
    """31 x 31 circular stamps: N = 961 is no multiple of 32 (nor of 2), so the
    unpadded record and the padded slot differ and the pair streams' pad
    elements are rebuilt by the load.  One image runs on the automatic team."""
    cases = [stamp_case(j, 0) for j in range(nimg)]
    gns = np.stack([c[0] for c in cases])
    psf = cases[0][1]
    bkgs = np.array([c[2] for c in cases])
    kw = {k: v for k, v in cases[0][3].items() if k not in ("flux", "betaParam")}
    kw.update(stop_criterion=1, flux=np.array([c[3]["flux"] for c in cases]),
              betaParams=[c[3]["betaParam"] for c in cases])
    whole = sgpmod.sgp_betaDiv_batch(gns, psf, bkgs, MAXIT=10, **kw)
    part, st, segs = split_run(sgpmod, "sgp_betaDiv", gns, psf, bkgs, [4], 10, kw)
    same(whole, part)
    assert st.shape == (31, 31) and st.layout["g"] - st.layout["x"] == 7696  # 961 * 8, padded to 16
    assert np.all(segs[0]["counters"][:, 5] == whole["counters"][:, 5])


# ---------------------------------------------------------------------- 3. teams
@pytest.mark.parametrize("name,team,maxit,cut", [("lin64_beta", 2, 12, 5), ("lin64_beta", 3, 12, 5),
                                                 ("lin256_kl", 32, 6, 3)])
def test_teams_split_equals_whole(sgpmod, name, team, maxit, cut):
    import _bsgp
    fx, gns, bkg, kw, fn = lin_case(name)
    kw.pop("MAXIT")
    kw.update(stop_criterion=1, team=team)
    whole = solver(sgpmod, fn)(gns, fx["psf"], bkg, MAXIT=maxit, **kw)
    part, st, segs = split_run(sgpmod, fn, gns, fx["psf"], bkg, [cut], maxit, kw)
    same(whole, part)
    for s in segs:
        assert np.all(s["counters"][:, 5] == team)
    assert np.all(st.header["T"] == team)
    other = {2: 3, 3: 2, 32: 5}[team]  # (a request above the geometry's cap of 32 would be cut to it)
    with pytest.raises(_bsgp.BsgpError, match="team") as e:
        sgpmod.sgp_resume(segs[0]["state"], maxit, team=other)
    assert e.value.code == _bsgp.BSGP_ERR_ARG


# ------------------------------------------------- 4. persistent solver, slot order
def six_images():
    fx = golden("ref_lin64_beta.npz")
    gn = fx["gn"].astype(np.float64)
    rng = np.random.default_rng(5)
    gns = np.stack([gn, np.roll(gn, 7, 0), gn[::-1].copy(), rng.poisson(gn).astype(np.float64),
                    np.roll(gn, 11, 1), gn.T.copy()])
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, alpha=10.0, ccd_sat_level=65000.0,
              use_original_SGP_Afunction=False, schedule_lr=True, adapt_beta=False, team=1,
              betaParams=[1.05, 0.97, 1.0, 1.02, 1.08, 0.99])
    return fx, gns, kw


@pytest.mark.parametrize("first,second", [(1, 1), (0, 1), (1, 0)])
def test_persistent_slot_order_split_equals_whole(sgpmod, first, second):
    fx, gns, kw = six_images()
    whole = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, MAXIT=12, persistent=1, **kw)
    part, _, _ = split_run(sgpmod, "sgp_betaDiv", gns, fx["psf"], 100.0, [5], 12, kw,
                           resume_kw=dict(persistent=second), first_kw=dict(persistent=first))
    same(whole, part)


# ------------------------- 5. persistent solver, ring: images stop at different times
def test_persistent_ring_segments_until_all_stopped(sgpmod):
    """The 8 float32 adaptive-beta stamps (seed 0), stop rule 3, MAXIT 500, in
    segments of 8 iterations.  The fixture's recorded iteration counts are 16,
    23, 18, 24, 24, 28, 25, 22: star 0 stops on the very iteration a segment
    ends with (rule and MAXIT on the same iteration), most stop in the third
    segment, two cross into the fourth.  Stopped images keep their outputs bit
    for bit through the later segments."""
    SEG = 8
    cases = [stamp_case(j, 0) for j in range(8)]
    ref_it = np.array([int(c[4]["iters"]) for c in cases])
    seg_of = (ref_it - 1) // SEG
    assert seg_of.min() < seg_of.max()  # (CPU-side: they do not all stop in one segment)
    gns = np.stack([c[0] for c in cases])
    assert gns.dtype == np.float32
    psf = cases[0][1]
    bkgs = np.array([c[2] for c in cases])
    kw = {k: v for k, v in cases[0][3].items() if k not in ("flux", "betaParam")}
    assert kw["stop_criterion"] == 3 and kw["adapt_beta"]
    kw.update(flux=np.array([c[3]["flux"] for c in cases]),
              betaParams=[c[3]["betaParam"] for c in cases], team=1, persistent=1)
    whole = sgpmod.sgp_betaDiv_batch(gns, psf, bkgs, MAXIT=500, **kw)
    it = whole["iters"]
    assert ((it - 1) // SEG).min() < ((it - 1) // SEG).max(), it
    out = sgpmod.sgp_betaDiv_batch(gns, psf, bkgs, MAXIT=SEG, return_state=True, **kw)
    m, nseg = SEG, 1
    while not out["state"].stopped.all():
        st = out["state"]
        stopped = st.stopped
        np.testing.assert_array_equal(stopped, it <= m)  # the rule's verdict, not MAXIT's
        sgpmod.sgp_betaDiv_batch(gns[::-1].copy(), psf, bkgs, MAXIT=3, **kw)
        m += SEG
        nseg += 1
        assert m <= 500
        prev, out = out, sgpmod.sgp_resume(st, m, return_state=True)
        for k in KEYS:  # stopped images: unchanged, bit for bit
            a, b = prev[k][stopped], out[k][stopped]
            if a.ndim == 2 and a.shape[1] != b.shape[1]:
                b = b[:, :a.shape[1]]
            np.testing.assert_array_equal(a, b, err_msg=k)
    assert nseg == (int(it.max()) - 1) // SEG + 1 and nseg > 2
    same(whole, out)


# ------------------------------------------------------------ 6. cooperative build
def test_cooperative_persistent_split_equals_whole(sgpmod):
    """Two 640 x 640 images (675-point grid: the 512-thread cooperative
    persistent build, as tests/test_gpu_persist.py reaches it)."""
    import _bsgp
    gn, psf, bkg, kw, fn, fx = crowded_case("crowded_beta")
    kw = dict(kw)
    b0 = kw.pop("betaParam")
    flux = kw.pop("flux") * (640 * 640) / (450 * 450)
    kw.pop("adapt_beta", None)
    kw.pop("MAXIT", None)
    g = np.pad(np.asarray(gn, dtype=np.float32), ((0, 190), (0, 190)), mode="reflect")
    bk = np.pad(np.asarray(bkg), ((0, 190), (0, 190)), mode="reflect")
    gns = np.stack([g, np.roll(g, 37, 0)]).astype(np.float64)
    plan = _bsgp.get_plan(640, 640, psf, _bsgp.BSGP_CONV_LINEAR_FILL)
    assert plan.P == plan.Q == 675
    kw.update(stop_criterion=1, team=1, persistent=1, flux=flux, betaParams=[b0, 1.02],
              adapt_beta=False)
    whole = sgpmod.sgp_betaDiv_batch(gns, psf, bk, MAXIT=4, **kw)
    part, st, _ = split_run(sgpmod, "sgp_betaDiv", gns, psf, bk, [2], 4, kw)
    same(whole, part)
    assert st.field("bkg").shape == (2, 640, 640)


# ------------------------------------------------------- 7. subset and permutation
def test_resume_subset_and_permutation(sgpmod):
    fx, gns, kw = six_images()
    gns, kw["betaParams"] = gns[:4], kw["betaParams"][:4]
    whole = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, MAXIT=12, **kw)
    first = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, MAXIT=5, return_state=True, **kw)
    sgpmod.sgp_betaDiv_batch(gns[::-1].copy(), fx["psf"], 100.0, MAXIT=3, **kw)
    part = sgpmod.sgp_resume(first["state"], 12, images=[3, 1])
    same(whole, part, rows=[3, 1])
    sgpmod.sgp_betaDiv_batch(gns[::-1].copy(), fx["psf"], 100.0, MAXIT=3, **kw)
    part = sgpmod.sgp_resume(first["state"][[3, 1]], 12)  # the same through __getitem__
    same(whole, part, rows=[3, 1])
    with pytest.raises(ValueError, match="images"):
        sgpmod.sgp_resume(first["state"], 12, images=[4])


# ------------------------------------------------------------- 8. disk round trip
CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
import numpy as np
import sgp
st = sgp.SolverState.load(sys.argv[1])
out = sgp.sgp_resume(st, 12)
for k in {keys!r}:
    np.save(sys.argv[2] + k + ".npy", out[k])
"""


def test_disk_round_trip_in_a_fresh_process(sgpmod, tmp_path):
    fx, gns, kw = six_images()
    gns, kw["betaParams"] = gns[:2], kw["betaParams"][:2]
    whole = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, MAXIT=12, **kw)
    first = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, MAXIT=5, return_state=True, **kw)
    path = str(tmp_path / "state.npz")
    first["state"].save(path)
    code = CHILD.format(root=ROOT, pkg=PKG, keys=KEYS)
    subprocess.run([sys.executable, "-c", code, path, str(tmp_path) + os.sep], check=True,
                   timeout=300)
    part = {k: np.load(str(tmp_path / (k + ".npy"))) for k in KEYS}
    same(whole, part)


# ------------------------------------------------------------------- 9. refusals
def test_refusals_name_the_field(sgpmod):
    import _bsgp
    fx, gns, kw = six_images()
    gns, kw["betaParams"] = gns[:2], kw["betaParams"][:2]
    psf = fx["psf"]
    first = sgpmod.sgp_betaDiv_batch(gns, psf, 100.0, MAXIT=5, return_state=True, **kw)
    st = first["state"]
    mode = _bsgp.BSGP_CONV_LINEAR_FILL

    def lib_resume(state, prm, H=64, W=64, storage="f64"):
        with _bsgp.lease_plan(H, W, psf, mode, storage=storage) as plan:
            return plan.resume(state.to_device().records, prm)

    for maxit in (5, 3):
        with pytest.raises(_bsgp.BsgpError, match="MAXIT") as e:
            sgpmod.sgp_resume(st, maxit)
        assert e.value.code == _bsgp.BSGP_ERR_ARG
    with pytest.raises(ValueError, match="gamma"):
        sgpmod.sgp_resume(st, 12, gamma=1e-3)
    prm = st.params()
    prm.MAXIT = 12
    prm.gamma = 1e-3
    with pytest.raises(_bsgp.BsgpError, match="gamma") as e:
        lib_resume(st, prm)
    assert e.value.code == _bsgp.BSGP_ERR_ARG
    prm.gamma = st.params().gamma
    with pytest.raises(_bsgp.BsgpError, match="storage") as e:
        lib_resume(st, prm, storage="f32")
    assert e.value.code == _bsgp.BSGP_ERR_ARG
    with pytest.raises(_bsgp.BsgpError, match="shape") as e:
        lib_resume(st, prm, H=48, W=48)
    assert e.value.code == _bsgp.BSGP_ERR_ARG
    bad = st.to_host()
    bad = _bsgp.SolverState(bad.records.copy(), bad.psf)
    bad.records[1, 0] ^= 0xFF
    with pytest.raises(ValueError, match="magic"):
        sgpmod.sgp_resume(bad, 12)
    with pytest.raises(_bsgp.BsgpError, match="magic") as e:
        lib_resume(bad, prm)
    assert e.value.code == _bsgp.BSGP_ERR_ARG
    with pytest.raises(ValueError, match="return_state"):
        sgpmod.sgp_betaDiv_batch(gns, psf, 100.0, MAXIT=5, devices=[0], return_state=True, **kw)
    # and the untouched state still resumes
    whole = sgpmod.sgp_betaDiv_batch(gns, psf, 100.0, MAXIT=12, **kw)
    same(whole, sgpmod.sgp_resume(st, 12))
