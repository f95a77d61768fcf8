"""The persistent solver's stream policy (bsgp_device.hpp "cache policy",
BSGP_STREAM_NT): classes of its global loads and stores are non-temporal, the
phase kernels stay plain.  A cache policy changes no arithmetic, so the
persistent solver (policy) and the phase kernels (plain) of the same library
must agree bit for bit on x, iters, discr, flags, beta_final and the counters,
at the smallest shapes that reach every access the policy rewrites: narrow and
wide operand loaders, a last row without a partner, a partly filled staging
instruction, the static 270-point plan, every line-search route, a resumed
solve, and tasks of one image handed from workgroup to workgroup with
non-temporal payloads.  MI355X tests.
"""
import numpy as np
import pytest

from conftest import golden, stamp_case

pytestmark = pytest.mark.gpu

KEYS = ("x", "iters", "discr", "flags", "beta_final", "counters")
SEEDS_256 = (10000, 10002, 10004)  # oracle/cpu_bench.make_stamp, C3 parameters

C3_KW = dict(init_recon=2, proj_type=1, stop_criterion=1, tol_convergence=1e-5, gamma=1e-4,
             beta=0.4, alpha=10.0, alpha_min=1e-5, alpha_max=1e5, M_alpha=3, tau=0.5, M=1,
             max_projs=1000, ccd_sat_level=65000.0, scale_data=True,
             use_original_SGP_Afunction=False, adapt_beta=False, lr=1e-3, lr_exp_param=0.1,
             schedule_lr=True, team=1)


@pytest.fixture(scope="module")
def sgpmod():
    import _bsgp
    _bsgp.require_gpu()
    import sgp
    return sgp


_CASES = {}


def case(shape):
    """(images [B, H, W] float64 with integer counts, psf, scalar backgrounds
    [B], keywords) of one shape; built once."""
    if shape in _CASES:
        return _CASES[shape]
    if shape == "31x31":
        # odd width: the narrow loaders; odd H: a last row without a partner
        # (two == false in gather_pair, stage_pair, store_pair); Qh = 16: a
        # partly filled stage_pair instruction; circular A
        cs = [stamp_case(j, 0) for j in range(4)]
        gns = np.stack([np.asarray(c[0], dtype=np.float64) for c in cs]
                       + [np.roll(np.asarray(c[0], dtype=np.float64), 3, 1) for c in cs])
        bkg = np.array([float(c[2]) for c in cs] * 2)
        kw = {k: v for k, v in cs[0][3].items() if k not in ("flux", "betaParam")}
        kw.update(stop_criterion=1, adapt_beta=False, MAXIT=25, team=1,
                  flux=np.array([float(c[3]["flux"]) for c in cs] * 2),
                  betaParams=[1.05, 0.97, 1.02, 0.99, 1.08, 1.01, 0.95, 1.03])
        out = (gns, cs[0][1], bkg, kw)
    elif shape in ("40x70", "41x70"):
        # even width: the wide loaders with their half_swap; not square; 41: odd H
        h = int(shape[:2])
        fx = golden("ref_c3stop3_s0.npz")
        g = fx["gn"].astype(np.float64)
        gns = np.stack([g[100:100 + h, 60:130], g[20:20 + h, 150:220], g[200:200 + h, 10:80],
                        g[150:150 + h, 100:170]])
        kw = dict(C3_KW, MAXIT=30, betaParams=[1.05, 0.97, 1.02, 1.08])
        out = (gns, fx["psf"], np.full(4, 100.0), kw)
    elif shape == "64x64":
        fx = golden("ref_lin64_beta.npz")
        g = fx["gn"].astype(np.float64)
        gns = np.stack([np.roll(g, 5 * i, 1) for i in range(8)])
        kw = dict(C3_KW, MAXIT=60, betaParams=[1.05, 0.97, 1.02, 0.99, 1.08, 1.01, 0.95, 1.03])
        out = (gns, fx["psf"], np.full(8, 100.0), kw)
    else:
        # "256x256": the timed workload's images and static 270-point plan
        # (Qh = 136: five staging instructions, the last one partial; kGCH
        # gathers; the padding-batch skip)
        import cpu_bench
        st = [cpu_bench.make_stamp(s, 256, 25, 200) for s in SEEDS_256]
        gns = np.stack([s[0] for s in st])
        kw = dict(C3_KW, MAXIT=40, betaParams=1.05)
        out = (gns, st[0][1], np.full(3, 100.0), kw)
    _CASES[shape] = out
    return out


def trials_of(out):
    return (np.asarray(out["flags"]) >> 8) & 0xffff


def assert_same(out, base, what):
    for k in KEYS:
        np.testing.assert_array_equal(out[k], base[k], err_msg=f"{k}: {what}")


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("bkg_kind", ["scalar", "map"])
@pytest.mark.parametrize("shape", ["31x31", "40x70", "41x70", "64x64", "256x256"])
def test_persistent_policy_equals_plain_phase_kernels(sgpmod, shape, bkg_kind, mode):
    """MODE 3 (float64 images) and MODE 4 (the same counts as float32 images),
    scalar backgrounds and background maps."""
    gns, psf, bkg, kw = case(shape)
    if mode == 4:
        gns = gns.astype(np.float32)
        assert np.array_equal(gns.astype(np.float64), case(shape)[0])
    if bkg_kind == "map":
        B, H, W = gns.shape
        yy, xx = np.mgrid[0:H, 0:W]
        ramp = 1.0 + 0.05 * np.sin(0.37 * yy + 0.1) * np.cos(0.23 * xx)
        bkg = bkg[:, None, None] * ramp[None]
    pers = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=1, **kw)
    plain = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=0, **kw)
    assert np.all(pers["counters"][:, 3] == 0) and np.all(plain["counters"][:, 3] == 0)
    assert_same(pers, plain, "persistent=1 against persistent=0")
    if shape == "64x64":
        # both line-search outcomes occur, so the fused pass, the replay and
        # the direct passes all ran
        t = trials_of(pers)[:, 1:int(pers["iters"].max()) + 1]
        assert (t == 1).any() and (t >= 2).any(), t


def test_handoff_between_workgroups_with_policy_payloads(sgpmod):
    """96 images of 40x70: consecutive iterations of an image run on workgroups
    of different XCDs, which read what the previous one stored."""
    gns, psf, bkg, kw = case("40x70")
    gns = np.concatenate([np.roll(gns, 2 * i, 2) for i in range(24)])
    kw = dict(kw, betaParams=list(kw["betaParams"]) * 24)
    bkg = np.full(len(gns), 100.0)
    pers = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=1, **kw)
    plain = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=0, **kw)
    assert len(gns) == 96 and np.all(pers["counters"][:, 3] == 0)
    assert_same(pers, plain, "96 images, persistent=1 against persistent=0")


def test_resumed_solve_equals_whole(sgpmod):
    """The 64x64 batch saved after 7 iterations and resumed to 20 equals the
    uninterrupted solve."""
    gns, psf, bkg, kw = case("64x64")
    kw = dict(kw)
    kw.pop("MAXIT")
    whole = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, MAXIT=20, persistent=1, **kw)
    for persistent in (1, 0):
        first = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, MAXIT=7, persistent=persistent,
                                         return_state=True, **kw)
        part = sgpmod.sgp_resume(first["state"], 20)
        for k in KEYS:
            w, p = whole[k], part[k]
            if k in ("discr", "flags") and w.shape[1] != p.shape[1]:
                n = min(w.shape[1], p.shape[1])
                w, p = w[:, :n], p[:, :n]
            np.testing.assert_array_equal(p, w, err_msg=f"{k}: persistent={persistent}")
