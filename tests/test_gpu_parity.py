"""Parity of the HIP path (through the C ABI) with the reference's golden
vectors and with the CPU oracle.  All tests need an MI355X.

Tolerances (north_star: "within 1e-5 relative fp64"):
  * operators A/AT, betaDiv family: 1e-12 relative (pure fp64 arithmetic,
    different FFT algorithm / summation order);
  * solves: relative L2 of x <= 1e-5 (the north-star bar) and discrepancy
    rtol 1e-7; iteration counts equal.  Observed differences are ~1e-10 for
    these run lengths (rounding-level differences amplify with
    iteration count; all fixtures stay within the <=75-iteration window).
"""
import os

import numpy as np
import pytest

from conftest import golden, ref_kwargs

pytestmark = pytest.mark.gpu

SOLVE_RTOL = 1e-5


@pytest.fixture(scope="module")
def B():
    import _bsgp
    _bsgp.require_gpu()
    return _bsgp


@pytest.fixture(scope="module")
def sgpmod(B):
    import sgp
    return sgp


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


# ----------------------------------------------------------------- operators
def test_circular_operator_matches_numpy(B, ngc):
    gn, psf, bkg, obj = ngc
    plan = B.get_plan(256, 256, psf, B.BSGP_CONV_CIRCULAR)
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 1, (3, 256, 256))
    TF = np.fft.fftn(np.fft.fftshift(psf))
    for tr in (False, True):
        out = plan.apply(B.to_dev(x), transpose=tr).cpu().numpy()
        for i in range(3):
            ref = np.real(np.fft.ifftn((np.conj(TF) if tr else TF) * np.fft.fftn(x[i])))
            assert rel(out[i], ref) < 1e-13


def test_linear_operator_matches_astropy(B):
    fx = golden("ref_linear_conv.npz")
    for i in range(int(fx["n"])):
        x, k = fx[f"x{i}"], fx[f"k{i}"]
        plan = B.get_plan(x.shape[0], x.shape[1], k, B.BSGP_CONV_LINEAR_FILL)
        a = plan.apply(B.to_dev(x[None])).cpu().numpy()[0]
        at = plan.apply(B.to_dev(x[None]), transpose=True).cpu().numpy()[0]
        assert rel(a, fx[f"A{i}"]) < 1e-12, (i, rel(a, fx[f"A{i}"]))
        assert rel(at, fx[f"AT{i}"]) < 1e-12, (i, rel(at, fx[f"AT{i}"]))


@pytest.mark.parametrize("linear", [True, False])
def test_operator_split_and_persistent_paths_agree(B, linear):
    """bsgp_apply_operator spreads few images over many workgroups (rows,
    columns, rows) and runs one persistent workgroup per image for many: the
    same transforms, so the same bits."""
    import cpu_bench
    psf = cpu_bench.gaussian_psf(25) if linear else np.fft.ifftshift(
        np.pad(cpu_bench.gaussian_psf(25), ((52, 51), (52, 51))))
    mode = B.BSGP_CONV_LINEAR_FILL if linear else B.BSGP_CONV_CIRCULAR
    plan = B.get_plan(128, 128, psf, mode)
    rng = np.random.default_rng(3)
    x = B.to_dev(rng.uniform(0, 1, (300, 128, 128)))  # 300 * 4 > 1024 slots: persistent
    for tr in (False, True):
        many = plan.apply(x, transpose=tr).cpu().numpy()
        for i in (0, 137, 299):
            one = plan.apply(x[i:i + 1].contiguous(), transpose=tr).cpu().numpy()[0]
            np.testing.assert_array_equal(one, many[i])


def test_operator_2048_matches_numpy(B):
    """One 2048x2048 image: cooperative (workgroup-wide) transforms, TF built
    over many workgroups, A/AT against numpy."""
    rng = np.random.default_rng(4)
    psf = np.zeros((2048, 2048))
    psf[1024 - 32:1024 + 32, 1024 - 32:1024 + 32] = rng.uniform(0, 1, (64, 64))
    psf /= psf.sum()
    plan = B.get_plan(2048, 2048, psf, B.BSGP_CONV_CIRCULAR)
    x = rng.uniform(0, 1, (2048, 2048))
    TF = np.fft.rfft2(np.fft.fftshift(psf))
    for tr in (False, True):
        out = plan.apply(B.to_dev(x[None]), transpose=tr).cpu().numpy()[0]
        ref = np.fft.irfft2((np.conj(TF) if tr else TF) * np.fft.rfft2(x), s=x.shape)
        assert rel(out, ref) < 1e-13


def test_small_plan_after_large_keeps_lds_limit(B):
    """The kernels' dynamic-LDS limit is shared by every plan and only rises:
    a 64x64 plan created after a 2048x2048 one (cooperative transforms, > 64 KiB
    of LDS) must leave the large plan's launches valid."""
    rng = np.random.default_rng(5)
    psf = np.zeros((2048, 2048))
    psf[1024 - 8:1024 + 8, 1024 - 8:1024 + 8] = rng.uniform(0, 1, (16, 16))
    psf /= psf.sum()
    big = B.Plan(2048, 2048, psf, B.BSGP_CONV_CIRCULAR)
    small = B.Plan(64, 64, np.full((5, 5), 1 / 25.0), B.BSGP_CONV_LINEAR_FILL)
    x = rng.uniform(0, 1, (2048, 2048))
    out = big.apply(B.to_dev(x[None])).cpu().numpy()[0]
    ref = np.fft.irfft2(np.fft.rfft2(np.fft.fftshift(psf)) * np.fft.rfft2(x), s=x.shape)
    assert rel(out, ref) < 1e-13
    xs = rng.uniform(0, 1, (64, 64))
    assert np.isfinite(small.apply(B.to_dev(xs[None])).cpu().numpy()).all()


def test_odd_circular_operator_fftshift_quirk(B):
    """31x31: fftshift puts the PSF centre at n-1."""
    psf = np.zeros((31, 31))
    psf[15, 15] = 1.0
    x = np.zeros((31, 31))
    x[5, 7] = 1.0
    plan = B.get_plan(31, 31, psf, B.BSGP_CONV_CIRCULAR)
    out = plan.apply(B.to_dev(x[None])).cpu().numpy()[0]
    assert abs(out[4, 6] - 1.0) < 1e-13 and abs(out.sum() - 1.0) < 1e-12


# ------------------------------------------------------------- projectDF
def test_projectdf_kats(B):
    import flux_conserve_proj as fcp
    fx = golden("ref_projectdf_kats.npz")
    for i in range(int(fx["ncases"])):
        b, scaling, sat, lam0, dl0, maxp = fx[f"meta{i}"]
        x = fcp.projectDF(np.float64(b), fx[f"c{i}"], fx[f"dia{i}"], scaling,
                          ccd_sat_level=None if np.isnan(sat) else sat, lambda_=lam0,
                          dlambda_=dl0, max_projs=int(maxp))
        ref = fx[f"x{i}"]
        scale = max(np.abs(ref).max(), 1e-300)
        assert np.all(np.abs(x - ref) <= 1e-9 * scale), (i, np.abs(x - ref).max() / scale)


# ---------------------------------------------------------- betaDiv family
def test_betadiv_family_kats(B, sgpmod):
    fx = golden("ref_betadiv_kats.npz")
    for i, b in enumerate(fx["betas"]):
        v = sgpmod.betaDiv(fx["y"], fx["x"], b)
        assert abs(v - fx[f"div{i}"]) <= 1e-12 * max(1.0, abs(fx[f"div{i}"])), (b, v)
        d = sgpmod.betaDivDeriv(fx["y"], fx["x"], b)
        # sgp.py:495 sums seven terms of size ~1/(b-1)^2 that cancel to O(1):
        # fp64 rounding of pow/log is amplified by that factor.
        atol = 1e-14 * max(1.0, 1.0 / (b - 1) ** 2) if b != 1 else 1e-14
        np.testing.assert_allclose(np.broadcast_to(d, fx["y"].shape), fx[f"deriv{i}"],
                                   rtol=1e-12, atol=atol)
    kat = sgpmod.betaDivDeriv(np.array([9.3, 2.5, 4.5, 7.9, 1.5]), np.array([1, 2, 4.5, 7.9, 1.5]),
                              1.5).sum()
    assert abs(kat - 24.6697) < 1e-4  # sgp.py:477-486
    TF = np.fft.fftn(np.fft.fftshift(fx["wrtY_psf"]))
    AT = lambda x: np.real(np.fft.ifftn(np.conj(TF) * np.fft.fftn(np.reshape(x, (16, 16))))).flatten()
    for i, b in enumerate(fx["wrtY_betas"]):
        g = sgpmod.betaDivDerivwrtY(AT, fx["wrtY_den"], fx["wrtY_img"].flatten(), b)
        np.testing.assert_allclose(g, fx[f"wrtY{i}"], rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------ solves
CIRC = ["ngc_kl27", "ngc_beta27", "ngc_beta_adapt12", "ngc_kl_proj20", "ngc_beta_proj20",
        "ngc_kl_stop2", "ngc_kl_stop3", "ngc_kl_stop4", "ngc_kl_noscale", "ngc_beta_stop3_flux"]


@pytest.mark.parametrize("name", CIRC)
def test_solve_matches_reference_ngc(name, sgpmod, ngc, capsys):
    gn, psf, bkg, obj = ngc
    fx = golden(f"ref_{name}.npz")
    kw = ref_kwargs(fx)
    x, it, discr, times, none = getattr(sgpmod, str(fx["fn"]))(gn, psf, bkg, **kw)
    assert none is None
    assert it == int(fx["iters"])
    assert len(discr) == len(fx["discr"]) == len(times)
    assert rel(x, fx["x"]) < SOLVE_RTOL, rel(x, fx["x"])
    np.testing.assert_allclose(discr, fx["discr"], rtol=1e-7)


def test_ngc_do_sampling_search_one_launch(sgpmod, ngc):
    """simulation_test_sgp.py:57-110 with do_sampling=True: the reference's 30
    adaptive-beta candidates (np.random.seed(42), normal(1, 0.05), MAXIT 27)
    as ONE batched launch through sgp_betaDiv_multistart with the test's own
    score, rel_err against the ground truth (:83-85): every candidate's rel_err
    and discrepancy against the unchanged reference's run, the reference's
    choice by its strict running minimum (:92-94), then the final fixed-beta
    run with that beta (:100-108) against the reference's x and rel_err."""
    gn, psf, bkg, obj = ngc
    fx = golden("ref_ngc_sampling.npz")
    kw = dict(init_recon=3, stop_criterion=1, MAXIT=27, lr=1e-3, lr_exp_param=0.1,
              schedule_lr=True)

    def relerr(x):
        e = x - obj
        return float(np.sqrt(np.sum(e * e) / np.sum(obj * obj)))

    betas = [float(b) for b in fx["betas"]]
    _, info = sgpmod.sgp_betaDiv_multistart(gn, psf, bkg, betas=betas, score=relerr,
                                            final_solve=False, adapt_beta=True, **kw)
    assert len(info["candidates"]) == 30
    for i, (x, it, discr, _, _) in enumerate(info["candidates"]):
        assert it == int(fx["iters"][i])
        assert abs(info["scores"][i] / fx["relerr"][i] - 1) < 1e-7, (i, info["scores"][i])
        np.testing.assert_allclose(discr, fx["discr"][i], rtol=1e-7)
    # the reference's pick (a 5.5e-3 relative gap to the runner-up)
    assert info["best_beta"] == float(fx["best_beta"])
    assert rel(info["candidates"][info["best"]][0], fx["best_x"]) < SOLVE_RTOL
    x, it, discr, _, _ = sgpmod.sgp_betaDiv(gn, psf, bkg, betaParam=info["best_beta"],
                                            adapt_beta=False, **kw)
    assert it == int(fx["final_iters"]) and rel(x, fx["final_x"]) < SOLVE_RTOL
    assert abs(relerr(x) / float(fx["final_relerr"]) - 1) < 1e-7
    np.testing.assert_allclose(discr, fx["final_discr"], rtol=1e-7)


def test_ngc_kl27_known_answer(sgpmod, ngc):
    """simulation_test_sgp.py:17-34: rel. error vs ground truth 0.137887788241."""
    gn, psf, bkg, obj = ngc
    x, it, discr, _, _ = sgpmod.sgp(gn, psf, bkg, init_recon=3, stop_criterion=1, MAXIT=27)
    relerr = np.sqrt(np.sum((x - obj) ** 2) / np.sum(obj * obj))
    assert abs(relerr - 0.137887788241) < 1e-7, relerr
    assert it == 27 and len(discr) == 28


@pytest.mark.parametrize("name", ["sat_kl332", "sat_beta332"])
def test_satellite_332_known_answer(sgpmod, name):
    """simulation_test_sgp.py:37-56 / 112-169: the satellite for 332
    iterations, rel. error vs ground truth 0.2904372552 (KL) and
    0.2910767378 (beta = 1.0001).  At 332 iterations the runs are chaotic
    (SURVEY §4): the reference itself, fed the observed image changed by one
    ulp per pixel (8 random-sign seeds, make_golden.py satellite), lands
    rel_err in [0.2900, 0.2956] (KL) / [0.2898, 0.2971] (beta) and moves x by
    up to 7.7e-2 / 6.8e-2.  The device's FFT and sums round differently, so
    its rel_err and x must lie within 1.5x that ensemble's largest deviation
    from the reference's run.

    How this bar came about: the first bar tried (round 4) was 3x the spread
    the reference itself shows with scipy.fft in place of numpy's FFT (2.1e-4
    KL / 3.2e-4 beta in rel_err); the device missed it (|d rel_err| 9.1e-4
    KL, 1.40e-3 beta; gpurun_out/r04b_tests.log), because one FFT swap is a
    single sample of the chaos, not its width.  The 1-ulp ensemble measures
    that width; by itself it pins little beyond "the same attractor".

    The non-chaotic part is pinned iteration by iteration (make_golden.py
    satellite_ens): the ensemble's discrepancies stay within 1e-7 of the
    reference's run through iteration 94 (KL) / 102 (beta); there the
    device's relative deviation from the reference's discrepancy must stay
    within 3x the ensemble's at the same iteration (floor 1e-10).  Measured:
    the device runs at ~1.4x the ensemble (KL: 6.2e-11 vs 4.4e-11 at
    iteration 50, 8.1e-8 vs 5.7e-8 at 94) -- its FFT and sums round
    differently at every step, not only once at the input."""
    from conftest import golden, satellite_case
    gn, psf, bkg, obj, kw, fn, fx = satellite_case(name)
    x, it, discr, _, _ = getattr(sgpmod, fn)(gn, psf, bkg, **kw)
    assert it == 332 and len(discr) == 333
    ens = golden(f"ref_{name}_ensdiscr.npz")
    k = int(ens["last_1e7"])
    assert k >= 90, k
    dev = np.abs(discr / fx["discr"] - 1)
    print(name, "device discrepancy deviation at 50/94/100/200/332:", dev[[50, 94, 100, 200, 332]],
          "ensemble:", ens["discr_dev"][[50, 94, 100, 200, 332]])
    bar = np.maximum(3.0 * ens["discr_dev"][:k + 1], 1e-10)
    over = np.nonzero(dev[:k + 1] > bar)[0]
    assert over.size == 0, (name, over[:5], dev[over[:5]], bar[over[:5]])
    relerr = float(np.sqrt(np.sum((x - obj) ** 2) / np.sum(obj * obj)))
    ref = float(fx["relerr"])
    spread = float(np.max(np.abs(fx["relerr_ulp_ensemble"] - ref)))
    xspread = float(np.max(fx["x_rel_ulp_ensemble"]))
    print(name, "rel_err", relerr, "reference", ref, "ensemble spread", spread, "x rel",
          rel(x, fx["x"]), "ensemble x rel", xspread)
    assert abs(relerr - ref) <= 1.5 * spread, (relerr, ref, spread)
    assert rel(x, fx["x"]) <= 1.5 * xspread, (rel(x, fx["x"]), xspread)


def test_stamp31_odd_size_adaptive_beta(sgpmod):
    fx = golden("ref_stamp31_beta_adapt.npz")
    x, it, discr, _, _ = sgpmod.sgp_betaDiv(fx["gn"], fx["psf"], np.float64(20.0), init_recon=2,
                                            stop_criterion=1, MAXIT=15, alpha=10.0,
                                            betaParam=1.01, adapt_beta=True)
    assert it == int(fx["iters"])
    assert rel(x, fx["x"]) < SOLVE_RTOL
    np.testing.assert_allclose(discr, fx["discr"], rtol=1e-7)


@pytest.mark.parametrize("name", ["lin64_kl", "lin64_beta", "lin256_beta", "lin256_kl",
                                  "lin64_beta_bmap"])
def test_solve_matches_reference_linear(name, sgpmod):
    fx = golden(f"ref_{name}.npz")
    kw = ref_kwargs(fx)
    if not np.isnan(fx["flux"]):
        kw["flux"] = np.float64(fx["flux"])
    bkg = fx["bkg"] if fx["bkg"].ndim else np.float64(fx["bkg"])
    x, it, discr, _, _ = getattr(sgpmod, str(fx["fn"]))(fx["gn"].astype(np.float64), fx["psf"],
                                                        bkg, **kw)
    assert it == int(fx["iters"])
    assert rel(x, fx["x"]) < SOLVE_RTOL, rel(x, fx["x"])
    np.testing.assert_allclose(discr, fx["discr"], rtol=1e-7)


@pytest.mark.parametrize("proj_cache", [0, 1])
@pytest.mark.parametrize("name", ["lin64_beta", "lin256_kl", "lin256_beta", "lin64_beta_bmap"])
def test_projection_pixel_lists_match_reference(name, proj_cache, sgpmod):
    """projectDF with and without the pixel lists: the same
    multiplier sequence (evaluation count E_p identical), the reference's
    iterates within the solve tolerance; with the lists most evaluations cost
    no full pass over the image."""
    fx = golden(f"ref_{name}.npz")
    kw = ref_kwargs(fx)
    if not np.isnan(fx["flux"]):
        kw["flux"] = np.float64(fx["flux"])
    gns = fx["gn"].astype(np.float64)[None]
    bkg = fx["bkg"][None] if fx["bkg"].ndim else float(fx["bkg"])
    fn = sgpmod.sgp_betaDiv_batch if str(fx["fn"]) == "sgp_betaDiv" else sgpmod.sgp_batch
    out = fn(gns, fx["psf"], bkg, team=1, proj_cache=proj_cache, **kw)
    it = int(out["iters"][0])
    assert it == int(fx["iters"])
    assert rel(out["x"][0], fx["x"]) < SOLVE_RTOL, rel(out["x"][0], fx["x"])
    np.testing.assert_allclose(out["discr"][0, :it + 1], fx["discr"], rtol=1e-7)
    c = out["counters"][0]
    if proj_cache:
        assert 0 < c[6] < c[0], c  # full passes < evaluations
    else:
        assert c[6] == c[0] and c[7] == 0, c


# --------------------------------------------------------- batch properties
@pytest.mark.parametrize("team", [1, 2])
def test_batch_is_bitwise_equal_to_single_solves(sgpmod, team):
    """Fixed team size (workgroups per image): a batch result never depends on
    its neighbours, bit for bit."""
    fx = golden("ref_lin64_beta.npz")
    gn = fx["gn"].astype(np.float64)
    rng = np.random.default_rng(5)
    gns = np.stack([gn, np.roll(gn, 7, 0), gn[::-1].copy(), rng.poisson(gn).astype(np.float64)])
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, MAXIT=12, alpha=10.0,
              ccd_sat_level=65000.0, use_original_SGP_Afunction=False, schedule_lr=True,
              adapt_beta=False, team=team)
    betas = [1.05, 0.97, 1.0, 1.02]
    out = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, betaParams=betas, **kw)
    assert np.all(out["counters"][:, 5] == team)
    for i in range(4):
        one = sgpmod.sgp_betaDiv_batch(gns[i:i + 1], fx["psf"], 100.0, betaParams=betas[i:i + 1],
                                       **kw)
        assert one["iters"][0] == out["iters"][i]
        np.testing.assert_array_equal(one["x"][0], out["x"][i])
        np.testing.assert_array_equal(one["discr"][0], out["discr"][i])


@pytest.mark.parametrize("name,teams", [("lin64_beta", [2, 3, 8]), ("lin256_kl", [5, 32]),
                                        ("lin256_beta", [7, 32])])
def test_team_sizes_match_reference(sgpmod, name, teams):
    """T workgroups cooperating on one image (team barriers, per-member
    partials): same iterates as the reference within the solve tolerance for
    every team size, and the team size actually used is reported."""
    fx = golden(f"ref_{name}.npz")
    kw = ref_kwargs(fx)
    if not np.isnan(fx["flux"]):
        kw["flux"] = np.float64(fx["flux"])
    bkg = float(fx["bkg"])
    gns = fx["gn"].astype(np.float64)[None]
    fn = sgpmod.sgp_betaDiv_batch if str(fx["fn"]) == "sgp_betaDiv" else sgpmod.sgp_batch
    for T in teams:
        out = fn(gns, fx["psf"], bkg, team=T, **kw)
        assert out["counters"][0, 5] == T
        assert out["counters"][0, 3] & 4 == 0
        it = int(out["iters"][0])
        assert it == int(fx["iters"])
        assert rel(out["x"][0], fx["x"]) < SOLVE_RTOL, (T, rel(out["x"][0], fx["x"]))
        np.testing.assert_allclose(out["discr"][0, :it + 1], fx["discr"], rtol=1e-7)


@pytest.mark.parametrize("T", [64, 65, 100, 255])
def test_c4_group_leader_team_sizes(sgpmod, T):
    """C4's field (2048^2, cooperative plan) at explicit team sizes around
    the flag-barrier cutover: 64 members take the flat flag
    barriers, 65 / 100 / 255 the eight group leaders with uneven groups
    (T % 8 = 1, 4, 7; 255 also polls wide reductions, kRedPollMax).
    The team size used is reported, no barrier timed out, and the discrepancy
    of the reference's own C4 run (make_golden.py c4) is met at every one of
    three iterations."""
    import cpu_bench
    fx = golden("ref_c4_maxit20.npz")
    gn, psf = cpu_bench.make_stamp(0, 2048, 64, 5000, circular=True)
    kw = ref_kwargs(fx)
    b = kw.pop("betaParam")
    kw["MAXIT"] = 3
    out = sgpmod.sgp_betaDiv_batch(gn[None], psf, 100.0, betaParams=b, team=T, **kw)
    assert out["counters"][0, 5] == T
    assert out["counters"][0, 3] & 4 == 0
    assert int(out["iters"][0]) == 3
    np.testing.assert_allclose(out["discr"][0, :4], fx["discr"][:4], rtol=1e-7)
    assert abs(out["x"][0].sum() / np.sum(gn - 100.0) - 1) < 1e-8


def test_team_size_clamped_to_barrier_words(sgpmod):
    """A team request above kMaxTeam (512, the barrier words and the group
    leaders' polls of bsgp_device.hpp) is clamped, never run."""
    import cpu_bench
    fx = golden("ref_c4_maxit20.npz")
    gn, psf = cpu_bench.make_stamp(0, 2048, 64, 5000, circular=True)
    kw = ref_kwargs(fx)
    b = kw.pop("betaParam")
    kw["MAXIT"] = 1
    out = sgpmod.sgp_betaDiv_batch(gn[None], psf, 100.0, betaParams=b, team=4096, **kw)
    assert 1 <= out["counters"][0, 5] <= 512
    assert out["counters"][0, 3] & 4 == 0


def test_auto_team_spreads_small_batches(sgpmod):
    """team=0 (default): a single image uses many workgroups, a batch as large
    as the CU count uses one each."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    fx = golden("ref_lin64_beta.npz")
    gn = fx["gn"].astype(np.float64)
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, MAXIT=3, alpha=10.0,
              ccd_sat_level=65000.0, use_original_SGP_Afunction=False)
    one = sgpmod.sgp_betaDiv_batch(gn[None], fx["psf"], 100.0, betaParams=[1.05], **kw)
    assert one["counters"][0, 5] > 1
    many = sgpmod.sgp_betaDiv_batch(np.broadcast_to(gn, (ncu, *gn.shape)).copy(), fx["psf"], 100.0,
                                    betaParams=1.05, **kw)
    assert np.all(many["counters"][:, 5] == 1)


def test_flux_conservation_and_positivity_full_batch(sgpmod):
    """BASELINE config C3 geometry (256x256, 25x25 PSF, linear A): size-independent
    properties on a 64-image batch: sum(x) == flux (proj_type=1), x >= 0,
    monotone discrepancy (M=1), finite outputs."""
    fx = golden("ref_lin256_beta.npz")
    gn = fx["gn"].astype(np.float64)
    gns = np.stack([np.roll(np.roll(gn, 3 * i, 0), 5 * i, 1) for i in range(64)])
    out = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, betaParams=1.05, init_recon=2,
                                   proj_type=1, stop_criterion=1, MAXIT=8, alpha=10.0,
                                   ccd_sat_level=65000.0, use_original_SGP_Afunction=False,
                                   schedule_lr=True, adapt_beta=False)
    x = out["x"]
    assert np.all(np.isfinite(x)) and np.all(x >= 0)
    flux = np.sum(gns - 100.0, axis=(1, 2))
    np.testing.assert_allclose(x.sum(axis=(1, 2)), flux, rtol=1e-9)
    assert np.all(out["iters"] == 8)
    d = out["discr"][:, :9]
    assert np.all(np.diff(d, axis=1) <= 1e-9 * np.abs(d[:, 1:]))


def test_c4_field_2048_matches_oracle(sgpmod):
    """BASELINE config C4 geometry: one 2048x2048 field, 64x64 PSF embedded at
    the centre, circular A (pow-2 FFT), beta-SGP; the numpy oracle on the same
    inputs (a few iterations keep the CPU side to seconds).  The solve runs
    as a team of workgroups (team=0 auto for a single image)."""
    import cpu_bench
    import sgp_oracle
    gn, psf = cpu_bench.make_stamp(0, 2048, 64, 5000, circular=True)
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, MAXIT=3, alpha=10.0,
              ccd_sat_level=65000.0, use_original_SGP_Afunction=True, schedule_lr=True,
              adapt_beta=False, betaParam=1.05)
    xr, itr, dr, _, _ = sgp_oracle.sgp_betaDiv(gn, psf, np.float64(100.0), **kw)
    x, it, d, _, _ = sgpmod.sgp_betaDiv(gn, psf, np.float64(100.0), **kw)
    assert it == itr
    assert rel(x, xr) < SOLVE_RTOL, rel(x, xr)
    np.testing.assert_allclose(d, dr, rtol=1e-7)


# ------------------------------------------------ the timed configuration
def test_bench_c3_path_exact(sgpmod):
    """bench.py's timed path itself (tests/bench_path.py): BASELINE config C3,
    1024 x 256x256 to MAXIT 100, team 1, the default sub-batch streams
    (4 here: this process runs with HIP's 4 hardware queues), gn_compact on;
    image 0 against the reference's 100-iteration run, every image's
    invariants, 8 sampled images bitwise equal to single-image solves."""
    import bench_path
    s = bench_path.check(100)
    assert s["streams"] == sgpmod.STREAMS_DEFAULT
    print(s)


def test_bench_c3_path_exact_8_queues():
    """The same checks as bench.py actually runs them: GPU_MAX_HW_QUEUES=8
    (set by bench.py before HIP starts), hence 8 sub-batch streams; a fresh
    process, since the variable is read when the runtime initialises."""
    import json
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([sys.executable, os.path.join(here, "bench_path.py"), "--maxit", "100"],
                       env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    s = json.loads(r.stdout.strip().splitlines()[-1])
    assert s["streams"] == 8 and s["hw_queues"] == "8", s
    print(s)


def test_gn_compact_is_bitwise_neutral(sgpmod):
    """gn_compact 1 (observed counts kept in f32, decoded on every read) and 0
    (f64 storage) give the same bits, for one-workgroup and team solves."""
    fx = golden("ref_lin64_beta.npz")
    gn = fx["gn"].astype(np.float64)
    gns = np.stack([gn, np.roll(gn, 9, 1), gn.T.copy()])
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, MAXIT=15, alpha=10.0,
              ccd_sat_level=65000.0, use_original_SGP_Afunction=False, schedule_lr=True,
              adapt_beta=False, betaParams=1.05)
    for team in (1, 4):
        a = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, team=team, gn_compact=1, **kw)
        b = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, team=team, gn_compact=0, **kw)
        np.testing.assert_array_equal(a["x"], b["x"])
        np.testing.assert_array_equal(a["discr"], b["discr"])


# ------------------------------------------------------------ multi-device API
def test_devices_sharding_is_bitwise_equal(sgpmod):
    """devices=[...] shards (image, beta) pairs over GPUs, one host thread per
    device.  On a one-GPU box: devices=[0] and devices=[0, 0]
    (two threads, two shards on the same GPU) give the plain batch's bits."""
    fx = golden("ref_lin64_beta.npz")
    gn = fx["gn"].astype(np.float64)
    gns = np.stack([np.roll(gn, 5 * i, 1) for i in range(6)])
    betas = [1.05, 0.97, 1.02, 0.99, 1.08, 1.01]
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, MAXIT=10, alpha=10.0,
              ccd_sat_level=65000.0, use_original_SGP_Afunction=False, schedule_lr=True,
              adapt_beta=False, team=1)
    plain = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, betaParams=betas, **kw)
    for devs in ([0], [0, 0]):
        sh = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, betaParams=betas, devices=devs, **kw)
        for key in ("x", "iters", "discr", "beta_final"):
            np.testing.assert_array_equal(sh[key], plain[key])


def test_profiled_solve_reports_every_kernel_class(sgpmod):
    """bsgp_solve_profiled (bench.py's per-kernel roofline): same results as a
    plain one-stream solve, and one launch of k_dir / k_ls / k_bb per
    iteration with positive spans."""
    fx = golden("ref_lin256_beta.npz")
    kw = ref_kwargs(fx)
    gns = np.stack([fx["gn"].astype(np.float64)] * 8)
    a = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, team=1, streams=1, persistent=0, **kw)
    b = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, team=1, profile=True, persistent=0, **kw)
    np.testing.assert_array_equal(a["x"], b["x"])
    it = int(kw["MAXIT"])
    # setup, dir, col (A), ls (+AT), bb; no persistent launch
    assert list(b["launches"]) == [1, it, it, it, it, 0]
    assert np.all(b["kernel_ms"][:5] > 0)
    c = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, team=1, profile=True, persistent=1, **kw)
    np.testing.assert_array_equal(a["x"], c["x"])
    # every setup and every iteration in one launch (the setups folded into
    # k_persist, DESIGN §3.4: no k_setup launch)
    assert list(c["launches"]) == [0, 0, 0, 0, 0, 1]
    assert c["kernel_ms"][0] == 0 and c["kernel_ms"][5] > 0
    # stop rule 3 keeps the ready ring, whose setups stay a k_setup launch
    d = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, team=1, profile=True, persistent=1,
                                 **dict(kw, stop_criterion=3, tol_convergence=1e-9))
    assert list(d["launches"]) == [1, 0, 0, 0, 0, 1]


# ------------------------------------------------------- float32 storage (C4)
def test_f32_storage_batch_within_1e3_of_reference(sgpmod):
    """storage='f32' (iteration vectors in float32 in HBM, float64 sums and
    scalars): the reference's lin256_beta run (SURVEY §8d C4 row tolerance,
    1e-3 for <= 20 iterations) for single-workgroup and team solves."""
    fx = golden("ref_lin256_beta.npz")
    kw = ref_kwargs(fx)
    gns = np.stack([fx["gn"].astype(np.float64)] * 3)
    for team in (1, 8):
        out = sgpmod.sgp_betaDiv_batch(gns, fx["psf"], 100.0, storage="f32", team=team, **kw)
        for i in range(3):
            assert int(out["iters"][i]) == int(fx["iters"])
            assert rel(out["x"][i], fx["x"]) < 1e-3, (team, rel(out["x"][i], fx["x"]))
            np.testing.assert_allclose(out["discr"][i, :11], fx["discr"], rtol=1e-3)
            assert abs(out["x"][i].sum() - np.sum(gns[i] - 100.0)) <= 1e-6 * np.sum(gns[i])


def test_c4_field_2048_f32_storage(sgpmod):
    """BASELINE config C4 (2048x2048, 64x64 PSF embedded, circular A, beta-SGP)
    with float32 storage: against the float64 oracle (5 iterations) at 1e-3
    (SURVEY §8d)."""
    import cpu_bench
    import sgp_oracle
    gn, psf = cpu_bench.make_stamp(0, 2048, 64, 5000, circular=True)
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, alpha=10.0, ccd_sat_level=65000.0,
              use_original_SGP_Afunction=True, schedule_lr=True, adapt_beta=False, betaParams=1.05)
    okw = {k: v for k, v in kw.items() if k != "betaParams"}
    xr, itr, dr, _, _ = sgp_oracle.sgp_betaDiv(gn, psf, np.float64(100.0), MAXIT=5, betaParam=1.05,
                                               **okw)
    o32 = sgpmod.sgp_betaDiv_batch(gn[None], psf, 100.0, storage="f32", MAXIT=5, **kw)
    assert int(o32["iters"][0]) == itr
    assert rel(o32["x"][0], xr) < 1e-3, rel(o32["x"][0], xr)
    np.testing.assert_allclose(o32["discr"][0], dr, rtol=1e-3)


@pytest.mark.parametrize("storage,tol", [("f64", 1e-7), ("f32", 1e-3)])
def test_c4_field_2048_maxit20_matches_reference(sgpmod, storage, tol):
    """BASELINE config C4 to MAXIT 20 against the reference itself
    (tests/golden/make_golden.py c4: discrepancy and trials of every
    iteration, sum(x), sum(x^2), four 64x64 windows of x and the whole field
    rounded to float32).  SURVEY §8d's
    bar for the float32-storage path is 1e-3 for <= 20 iterations; the
    float64 path is held to the north-star 1e-5 on x and rtol 1e-7 on the
    discrepancy.  The inputs are rebuilt with the fixture's generator."""
    import cpu_bench
    from conftest import compare_trials
    fx = golden("ref_c4_maxit20.npz")
    gn, psf = cpu_bench.make_stamp(0, 2048, 64, 5000, circular=True)
    np.testing.assert_allclose([gn.sum(), np.sum(gn * gn)], [fx["gn_sum"], fx["gn_x2"]], rtol=0)
    kw = ref_kwargs(fx)
    b = kw.pop("betaParam")
    out = sgpmod.sgp_betaDiv_batch(gn[None], psf, 100.0, storage=storage, betaParams=b, **kw)
    it = int(out["iters"][0])
    assert it == int(fx["iters"]) == 20
    x = out["x"][0]
    np.testing.assert_allclose(out["discr"][0, :it + 1], fx["discr"], rtol=tol)
    xt = max(tol, 1e-5)
    for j, (r, c) in enumerate(fx["wins"]):
        w = x[r:r + 64, c:c + 64]
        assert rel(w, fx[f"win{j}"]) < xt, (storage, j, rel(w, fx[f"win{j}"]))
    np.testing.assert_allclose([x.sum(), np.sum(x * x)], [fx["xsum"], fx["x2"]], rtol=xt)
    # the whole field, pixel by pixel, against the reference's x rounded to
    # float32 (x32): the fixture's own rounding is 2^-24 |x32| per pixel
    x32 = fx["x32"].astype(np.float64)
    assert rel(x, x32) < xt, (storage, rel(x, x32))
    d = np.abs(x - x32) - 2.0 ** -24 * np.abs(x32)
    scale = np.abs(x32) + 1e-7 * np.abs(x32).max()
    worst = float(np.max(d / scale))
    zeros = int(np.sum((x == 0) != (x32 == 0)))
    print(f"c4 {storage}: full-field rel {rel(x, x32):.3e}, worst pixel {worst:.3e}, "
          f"zero-pattern mismatches {zeros}")
    if storage == "f64":
        # every pixel within 1e-7 of itself (floor 1e-7 of the peak) beyond
        # the fixture's float32 rounding, and the same pixels projected to
        # zero; measured: worst 0 (all deviations below 2^-24), rel 2.4e-8
        assert worst <= 1e-7 and zeros == 0, (worst, zeros)
        compare_trials((np.asarray(out["flags"][0, 1:it + 1]) >> 8), fx["trials"], "c4")
