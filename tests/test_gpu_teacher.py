"""Teacher-forced one-step checks: a solver state captured at the
head of iteration k inside the UNCHANGED reference (tests/golden/ref_states.npz,
made by tests/golden/make_golden_states.py) is turned into a record with
SolverState.from_arrays, the device runs exactly iteration k from it, and the
result is held against the reference's own state at the head of iteration
k + 1.  No trajectory is followed, so the bars do not grow with k: this pins
iterations beyond the chaos horizon, where whole runs can only be
held to an ensemble width.  MI355X tests.

Bars (the project's own for whole short solves; one step cannot need more):
x within SOLVE_RTOL (relative L2), fv and the discrepancy at rtol 1e-7, alpha,
tau, beta and lr at rtol 1e-9, the line-search trial count through
conftest.compare_trials.  Measured one-step deviations are listed in DESIGN §4.
"""
import ast

import numpy as np
import pytest

from conftest import compare_trials, golden

pytestmark = pytest.mark.gpu

SOLVE_RTOL = 1e-5
CASES = [("kl", 25), ("kl", 150), ("beta", 30), ("beta", 150), ("adapt", 10)]


@pytest.fixture(scope="module")
def states():
    return golden("ref_states.npz")  # loaded once, shared, never written


@pytest.fixture(scope="module")
def sgpmod():
    import _bsgp
    _bsgp.require_gpu()
    import sgp
    return sgp


def record(sgpmod, z, name, k):
    """The reference's locals at the head of iteration k as a solver-state
    record.  pw = den**(beta-1) and konst = sum(s*gn**beta) are evaluated in
    numpy as oracle/sgp_oracle.py evaluates the reference's powers (``**``)."""
    import _bsgp
    p = f"{name}_k{k}_"
    fn = str(z[f"{name}_fn"])
    kw = ast.literal_eval(str(z[f"{name}_kwargs"]))
    s = dict(zip([str(n) for n in z[p + "names"]], z[p + "scalars"]))
    beta_obj = fn == "sgp_betaDiv"
    prm = sgpmod.state_params("beta" if beta_obj else "kl", MAXIT=k, team=1, **kw)
    gn, x_tf, bkg = z[f"{name}_gn"], z[p + "x_tf"], float(z[p + "bkg"])
    extra = {}
    if beta_obj:
        b = s["betaParam"]
        extra = dict(pw=(x_tf + bkg) ** (b - 1), beta=b, lr=s["lr"], init_lr=kw["lr"],
                     konst=np.sum(1 / (b * (b - 1)) * gn ** b))
    st = _bsgp.SolverState.from_arrays(
        z["psf"], prm, z[p + "x"], z[p + "g"], x_tf, gn, bkg=bkg, iters_done=k - 1,
        alpha=s["alpha"], tau=s["tau"], fv=s["fv"], flux=s["flux"], scaling=s["scaling"],
        x_low=s["X_low_bound"], x_upp=s["X_upp_bound"], tol=float(z[p + "tol"]),
        Valpha=z[p + "Valpha"], Fold=z[p + "Fold"], conv_mode=_bsgp.BSGP_CONV_CIRCULAR, **extra)
    return st, s, dict(zip([str(n) for n in z[p + "names"]], z[p + "next"]))


def one_step(sgpmod, z, name, k):
    """Deviations of the device's iteration k from the reference's."""
    st, s, nxt = record(sgpmod, z, name, k)
    out = sgpmod.sgp_resume(st, k, return_state=True)
    new = out["state"]
    h = new.header[0]
    assert int(out["iters"][0]) == k and list(new.iters_done) == [k]
    x = new.field("x")[0]
    xr = z[f"{name}_k{k}_x_next"]
    r = lambda a, b: abs(a / b - 1)  # noqa: E731
    dev = {"x": float(np.linalg.norm(x - xr) / np.linalg.norm(xr)),
           "fv": r(h["fv"], nxt["fv"]),
           "discr": r(out["discr"][0, k], 2 / xr.size * s["scaling"] * nxt["fv"]),
           "alpha": r(h["alpha"], nxt["alpha"]), "tau": r(h["tau"], nxt["tau"])}
    if "betaParam" in nxt:
        dev["beta"] = r(h["beta"], nxt["betaParam"])
        dev["lr"] = r(h["lr"], nxt["lr"])
    trials = (int(out["flags"][0, k]) >> 8) & 0xFFFF
    # the history rows before k are the record's (zeros here), the state goes on
    assert not new.stopped.any() and out["counters"][0, 1] == trials
    return dev, trials, int(z[f"{name}_k{k}_trials"])


@pytest.mark.parametrize("name,k", CASES)
def test_one_iteration_from_a_reference_state(sgpmod, states, name, k):
    dev, trials, ref_trials = one_step(sgpmod, states, name, k)
    print(f"teacher {name} k={k}: " + " ".join(f"{a}={v:.3e}" for a, v in dev.items())
          + f" trials={trials} (reference {ref_trials})")
    assert dev["x"] < SOLVE_RTOL, dev
    assert dev["fv"] < 1e-7 and dev["discr"] < 1e-7, dev
    for a in ("alpha", "tau", "beta", "lr"):
        if a in dev:
            assert dev[a] < 1e-9, (a, dev)
    compare_trials([trials], [ref_trials], what=f"{name} k={k}")
