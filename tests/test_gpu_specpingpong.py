"""The speculative fused pass of the persistent line search on two spectra
(ls_phase, SolveArgs::spec2).  After an accepted lam = 1 the search reads
A(d)'s rows from the slot's spectrum, writes w's rows to the second spectrum
and stores no d_tf.  An accepted first trial selects the second spectrum for
AT's column pass and for bb_phase (ImgState::par_spec); a rejected one finds
A(d) intact and reruns the ordinary pass 1, which is not counted as a pass or
a trial.  None of this may change a bit: compared are x, discr, iters,
beta_final, the per-iteration trial counts in flags and all counters, between
BSGP_LS_PREDICT 0 (never speculates), 1 (default) and 2 (speculates in every
iteration, so every iteration that does not accept lam = 1 takes the rerun),
and against the phase kernels, which carry no prediction.  MI355X tests.
"""
import numpy as np
import pytest

from conftest import golden, stamp_case

pytestmark = pytest.mark.gpu

KEYS = ("x", "iters", "discr", "flags", "beta_final", "counters")
# bench-generator seeds (oracle/cpu_bench.make_stamp, C3 parameters): the
# oracle's replay (tools/ls_predict_replay.py) has first-trial misses at
# iterations 13, 15-17, 23-24 and 9-10 and the switch to stagnation at 35-46
SEEDS_256 = (10000, 10001, 10002)

C3_KW = dict(init_recon=2, proj_type=1, stop_criterion=1, tol_convergence=1e-5, gamma=1e-4,
             beta=0.4, alpha=10.0, alpha_min=1e-5, alpha_max=1e5, M_alpha=3, tau=0.5, M=1,
             max_projs=1000, ccd_sat_level=65000.0, scale_data=True,
             use_original_SGP_Afunction=False, adapt_beta=False, lr=1e-3, lr_exp_param=0.1,
             schedule_lr=True, team=1)

_CASES = {}


@pytest.fixture(scope="module")
def sgpmod():
    import _bsgp
    _bsgp.require_gpu()
    import sgp
    return sgp


def case(shape):
    """(images [B, H, W], psf, scalar backgrounds [B], keywords); built once."""
    if shape in _CASES:
        return _CASES[shape]
    if shape == "31x31":  # odd N, circular A, runtime geometry
        cs = [stamp_case(j, 0) for j in range(4)]
        gns = np.stack([np.asarray(c[0], dtype=np.float64) for c in cs]
                       + [np.roll(np.asarray(c[0], dtype=np.float64), 3, 1) for c in cs])
        bkg = np.array([float(c[2]) for c in cs] * 2)
        kw = {k: v for k, v in cs[0][3].items() if k not in ("flux", "betaParam")}
        kw.update(stop_criterion=1, adapt_beta=False, MAXIT=25, team=1,
                  flux=np.array([float(c[3]["flux"]) for c in cs] * 2),
                  betaParams=[1.05, 0.97, 1.02, 0.99, 1.08, 1.01, 0.95, 1.03])
        out = (gns, cs[0][1], bkg, kw)
    elif shape == "40x70":  # even width, not square, runtime geometry
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
        kw = dict(C3_KW, MAXIT=20, betaParams=[1.05, 0.97, 1.02, 0.99, 1.08, 1.01, 0.95, 1.03])
        out = (gns, fx["psf"], np.full(8, 100.0), kw)
    else:  # "256x256": the timed workload's images; the only shape of the static plan
        import cpu_bench
        st = [cpu_bench.make_stamp(s, 256, 25, 200) for s in SEEDS_256]
        gns = np.stack([s[0] for s in st])
        kw = dict(C3_KW, MAXIT=45, betaParams=1.05)
        out = (gns, st[0][1], np.full(3, 100.0), kw)
    _CASES[shape] = out
    return out


def trials_of(out):
    """Line-search trials of iterations 1 .. max(iters), [B, iterations]."""
    t = (np.asarray(out["flags"]) >> 8) & 0xffff
    return t[:, 1:int(np.asarray(out["iters"]).max()) + 1]


def assert_same(out, base, what):
    for k in KEYS:
        np.testing.assert_array_equal(out[k], base[k], err_msg=f"{k}: {what}")


def solve_all(sgpmod, monkeypatch, gns, psf, bkg, kw, **extra):
    """BSGP_LS_PREDICT 0, 1 and 2, persistent solver and phase kernels: all
    equal to the first solve (value 0, persistent) bit for bit."""
    base = None
    for v in ("0", "1", "2"):
        monkeypatch.setenv("BSGP_LS_PREDICT", v)  # (part of the plan pool's key)
        for persistent in (1, 0):
            out = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=persistent, **extra, **kw)
            assert np.all(out["counters"][:, 3] == 0)
            if base is None:
                base = out
            else:
                assert_same(out, base, f"BSGP_LS_PREDICT={v}, persistent={persistent}")
    return base


def assert_hits_and_misses(t):
    """From the trial counts (the same under every knob value): with the
    default prediction an iteration after a one-trial iteration speculates."""
    one = t[:, :-1] == 1
    # a speculative accept followed by another: the second spectrum is
    # selected in two iterations running (the first of the two iterations
    # speculates because its predecessor took one trial as well)
    assert (one[:, :-1] & one[:, 1:] & (t[:, 2:] == 1)).any(), t
    # a real miss after a real accept: >= 2 trials directly after one trial, so
    # the rerun of pass 1 ran behind a speculation
    assert (one & (t[:, 1:] >= 2)).any(), t


@pytest.mark.parametrize("shape", ["256x256", "40x70", "31x31"])
def test_ping_pong_gives_the_same_bits(sgpmod, monkeypatch, shape):
    gns, psf, bkg, kw = case(shape)
    base = solve_all(sgpmod, monkeypatch, gns, psf, bkg, kw)
    if shape == "256x256":
        assert sgpmod.last_static_geo() is False  # (the last solve ran the phase kernels)
        monkeypatch.setenv("BSGP_LS_PREDICT", "1")
        sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=1, **kw)
        assert sgpmod.last_static_geo() is True
    assert_hits_and_misses(trials_of(base))


def test_runtime_geometry_at_256(sgpmod, monkeypatch):
    """The 256 x 256 plan on the runtime-geometry phases (static_geo=0) against
    the compile-time ones, with and without speculation."""
    gns, psf, bkg, kw = case("256x256")
    monkeypatch.setenv("BSGP_LS_PREDICT", "0")
    base = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=1, static_geo=1, **kw)
    assert sgpmod.last_static_geo() is True
    for v in ("1", "2"):
        monkeypatch.setenv("BSGP_LS_PREDICT", v)
        for sg in (0, 1):
            out = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=1, static_geo=sg, **kw)
            assert sgpmod.last_static_geo() is bool(sg)
            assert_same(out, base, f"BSGP_LS_PREDICT={v}, static_geo={sg}")


def test_resume_after_an_odd_number_of_speculative_accepts(sgpmod, monkeypatch):
    """64 x 64, always speculating: saved where image 0 has accepted an odd
    number of speculations (the second x_tf / pw pair is current and the last
    AT(w) went through the second spectrum), resumed to the end: equal to the
    unsplit solve without prediction."""
    gns, psf, bkg, kw = case("64x64")
    kw = dict(kw)
    total = kw.pop("MAXIT")
    monkeypatch.setenv("BSGP_LS_PREDICT", "0")
    whole = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, MAXIT=total, persistent=1, **kw)
    acc = np.cumsum(trials_of(whole)[0] == 1)  # value 2: every one-trial iteration is a speculative accept
    cut = [n for n in range(3, total - 2) if acc[n - 1] % 2 == 1]
    assert cut, acc
    for v in ("1", "2"):
        monkeypatch.setenv("BSGP_LS_PREDICT", v)
        first = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, MAXIT=cut[0], persistent=1,
                                         return_state=True, **kw)
        part = sgpmod.sgp_resume(first["state"], total)
        for k in KEYS:
            w, p = whole[k], part[k]
            if k in ("discr", "flags") and w.shape[1] != p.shape[1]:
                n = min(w.shape[1], p.shape[1])
                w, p = w[:, :n], p[:, :n]
            np.testing.assert_array_equal(p, w, err_msg=f"{k}: BSGP_LS_PREDICT={v}")


def test_second_batch_on_a_used_plan(sgpmod, monkeypatch):
    """Two different batches back to back on one plan: the second equals its
    solve on a fresh plan (nothing of the first batch's spectrum selection or
    buffer parity survives the setup)."""
    import _bsgp
    gns, psf, bkg, kw = case("64x64")
    other = np.ascontiguousarray(np.roll(gns, 7, 2)[::-1])
    monkeypatch.setenv("BSGP_LS_PREDICT", "2")
    _bsgp._pool.clear()
    sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=1, **kw)
    second = sgpmod.sgp_betaDiv_batch(other, psf, bkg, persistent=1, **kw)
    assert sum(len(v) for v in _bsgp._pool.values()) == 1  # the same plan served both
    _bsgp._pool.clear()
    fresh = sgpmod.sgp_betaDiv_batch(other, psf, bkg, persistent=1, **kw)
    assert_same(second, fresh, "used plan against fresh plan")
    t = trials_of(fresh)
    assert (t == 1).any() and (t >= 2).any(), t
