"""The line search's outcome prediction (ls_phase, BSGP_LS_PREDICT; the
persistent solver's build).  After an accepted lam = 1 the search runs pass 1
and the accept as one speculative fused row pass; a replay pass supplies the
moments and the second trial's sums when the first trial then fails.  A
prediction only chooses the route, so every value of the knob gives the same
bits: 0 never predicts, 1 (default) predicts accepts from the last step, 2
always predicts an accept (every iteration that does not accept lam = 1 takes
the replay), 3 always predicts a stagnation (pass 1 without the second trial's
sums; the replay where the closed form does not cover that trial), 4 and 5
predict stagnations from the last step as well / only.  Compared: x, discr,
iters, beta_final, the per-iteration trial counts in flags and all counters
(E_ls, ls_series, ls_passes among them), between the knob's values and against
the phase kernels, which carry no prediction.  MI355X tests.
"""
import numpy as np
import pytest

from conftest import golden, stamp_case

pytestmark = pytest.mark.gpu

KEYS = ("x", "iters", "discr", "flags", "beta_final", "counters")
# bench-generator seeds (oracle/cpu_bench.make_stamp, C3 parameters) whose
# searches leave the lam = 1 accepts for stagnation at iterations 35, 46 and
# 31 (tools/ls_predict_replay.py --maxit 100), mixed iterations before
SEEDS_256 = (10000, 10002, 10004)


@pytest.fixture(scope="module")
def sgpmod():
    import _bsgp
    _bsgp.require_gpu()
    import sgp
    return sgp


C3_KW = dict(init_recon=2, proj_type=1, stop_criterion=1, tol_convergence=1e-5, gamma=1e-4,
             beta=0.4, alpha=10.0, alpha_min=1e-5, alpha_max=1e5, M_alpha=3, tau=0.5, M=1,
             max_projs=1000, ccd_sat_level=65000.0, scale_data=True,
             use_original_SGP_Afunction=False, adapt_beta=False, lr=1e-3, lr_exp_param=0.1,
             schedule_lr=True, team=1)

_CASES = {}


def case(shape):
    """(images [B, H, W] float64 with integer counts, psf, scalar backgrounds
    [B], keywords) of one shape; built once."""
    if shape in _CASES:
        return _CASES[shape]
    if shape == "31x31":  # odd width and odd N, circular A, runtime transform plan
        cs = [stamp_case(j, 0) for j in range(4)]
        gns = np.stack([np.asarray(c[0], dtype=np.float64) for c in cs]
                       + [np.roll(np.asarray(c[0], dtype=np.float64), 3, 1) for c in cs])
        bkg = np.array([float(c[2]) for c in cs] * 2)
        kw = {k: v for k, v in cs[0][3].items() if k not in ("flux", "betaParam")}
        kw.update(stop_criterion=1, adapt_beta=False, MAXIT=25, team=1,
                  flux=np.array([float(c[3]["flux"]) for c in cs] * 2),
                  betaParams=[1.05, 0.97, 1.02, 0.99, 1.08, 1.01, 0.95, 1.03])
        out = (gns, cs[0][1], bkg, kw)
    elif shape == "40x70":  # even width, not square
        fx = golden("ref_c3stop3_s0.npz")
        g = fx["gn"].astype(np.float64)
        gns = np.stack([g[100:140, 60:130], g[20:60, 150:220], g[200:240, 10:80],
                        g[150:190, 100:170]])
        kw = dict(C3_KW, MAXIT=30, betaParams=[1.05, 0.97, 1.02, 1.08])
        out = (gns, fx["psf"], np.full(4, 100.0), kw)
    elif shape == "64x64":
        fx = golden("ref_lin64_beta.npz")
        g = fx["gn"].astype(np.float64)
        gns = np.stack([np.roll(g, 5 * i, 1) for i in range(8)])
        kw = dict(C3_KW, MAXIT=60, betaParams=[1.05, 0.97, 1.02, 0.99, 1.08, 1.01, 0.95, 1.03])
        out = (gns, fx["psf"], np.full(8, 100.0), kw)
    else:  # "256x256": the timed workload's images and static 270-point plan
        import cpu_bench
        st = [cpu_bench.make_stamp(s, 256, 25, 200) for s in SEEDS_256]
        gns = np.stack([s[0] for s in st])
        kw = dict(C3_KW, MAXIT=70, betaParams=1.05)
        out = (gns, st[0][1], np.full(3, 100.0), kw)
    _CASES[shape] = out
    return out


def trials_of(out):
    return (np.asarray(out["flags"]) >> 8) & 0xffff


def solve_all(sgpmod, monkeypatch, gns, psf, bkg, kw, values=("0", "1", "2", "3", "4", "5")):
    """The solve under every knob value, persistent solver and phase kernels;
    everything must equal value 0's persistent solve bit for bit."""
    base = None
    for v in values:
        monkeypatch.setenv("BSGP_LS_PREDICT", v)  # (part of the plan pool's key: a fresh plan)
        for persistent in (1, 0):
            out = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=persistent, **kw)
            assert np.all(out["counters"][:, 3] == 0)
            if base is None:
                base = out
                continue
            for k in KEYS:
                np.testing.assert_array_equal(out[k], base[k],
                                              err_msg=f"{k}: BSGP_LS_PREDICT={v}, "
                                                      f"persistent={persistent}")
    return base


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("bkg_kind", ["scalar", "map"])
@pytest.mark.parametrize("shape", ["31x31", "40x70", "64x64", "256x256"])
def test_every_prediction_gives_the_same_bits(sgpmod, monkeypatch, shape, bkg_kind, mode):
    """MODE 3 (float64 images) and MODE 4 (the same counts as float32 images:
    the objective's float32-rounded factors), scalar backgrounds and maps."""
    gns, psf, bkg, kw = case(shape)
    if mode == 4:
        gns = gns.astype(np.float32)
        assert np.array_equal(gns.astype(np.float64), case(shape)[0])
    if bkg_kind == "map":
        B, H, W = gns.shape
        yy, xx = np.mgrid[0:H, 0:W]
        ramp = 1.0 + 0.05 * np.sin(0.37 * yy + 0.1) * np.cos(0.23 * xx)
        bkg = bkg[:, None, None] * ramp[None]
    base = solve_all(sgpmod, monkeypatch, gns, psf, bkg, kw)
    t = trials_of(base)[:, 1:int(base["iters"].max()) + 1]
    # both outcomes occur, so the always-accept and always-stagnate settings
    # were wrong somewhere and the repairs ran
    assert (t == 1).any() and (t >= 2).any(), t
    if shape == "256x256" and bkg_kind == "scalar":
        # the oracle's replay of these seeds: accepts at first, stagnation
        # (conftest.STAGNATION_FLOOR trials or more) from iteration 46 at the latest
        assert (t[:, :5] == 1).all() and (t[:, -5:] >= 16).all(), t


@pytest.mark.parametrize("value", ["1", "2", "3"])
def test_resumed_solve_under_prediction_equals_whole(sgpmod, monkeypatch, value):
    """A 64x64 batch saved after 7 iterations (an odd number of speculative
    accepts leaves the second x_tf / pw pair current: the record takes it from
    there and the resumed solve starts on the first) and resumed to 20 equals
    the uninterrupted solve without prediction.  The record does not carry the
    last step: a resumed image starts from lam = 0."""
    gns, psf, bkg, kw = case("64x64")
    kw = dict(kw)
    kw.pop("MAXIT")
    monkeypatch.setenv("BSGP_LS_PREDICT", "0")
    whole = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, MAXIT=20, persistent=1, **kw)
    monkeypatch.setenv("BSGP_LS_PREDICT", value)
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
