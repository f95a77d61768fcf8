"""Generate tests/golden/ref_states.npz: solver states captured inside the
UNCHANGED reference, for the teacher-forced one-step tests
(tests/test_gpu_teacher.py).

Run ONLY where the reference is present (it is imported from make_golden.py's
REF, with the same import stubs):

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_states.py

The reference's sgp() / sgp_betaDiv() run under ``sys.settrace``.  Whenever
the loop head ``prev_x = x.copy()`` (restoration/sgp.py:303 / :750) is about to
execute with iter_ == k or k + 1, the frame's locals are copied: at k the
state an iteration starts from (x, g, x_tf, gn, bkg, alpha, tau, Valpha, Fold,
fv, the bounds, flux, scaling, tol, and betaParam / lr for the beta variant),
at k + 1 what that one iteration made of it.  The line-search trials of
iteration k are the executions of the Armijo test (sgp.py:336 / :784) between
the two.  Nothing of the reference is modified.

All cases are 64 x 64 circular with a 64 x 64 Gaussian PSF (the stub import
path needs no astropy): KL without projection at k = 25 and 150, beta = 1.05
with the flux projection and saturation at k = 30 and 150, adaptive beta at
k = 10.
"""
import linecache
import os
import sys
import tempfile

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import gaussian_psf, import_reference, synth_field  # noqa: E402

CASES = {
    "kl": ("sgp", dict(init_recon=2, proj_type=0, stop_criterion=1, alpha=10.0), (25, 150)),
    "beta": ("sgp_betaDiv", dict(init_recon=2, proj_type=1, stop_criterion=1, alpha=10.0,
                                 ccd_sat_level=65000.0, betaParam=1.05, lr=1e-3, lr_exp_param=0.1,
                                 schedule_lr=True, adapt_beta=False), (30, 150)),
    "adapt": ("sgp_betaDiv", dict(init_recon=2, proj_type=1, stop_criterion=1, alpha=10.0,
                                  ccd_sat_level=65000.0, betaParam=1.02, lr=1e-3,
                                  lr_exp_param=0.1, schedule_lr=True, adapt_beta=True), (10,)),
}
VECS = ("x", "g", "x_tf")
SCALARS = ("alpha", "tau", "fv", "X_low_bound", "X_upp_bound", "flux", "scaling")


def capture(sgp, fn, gn, psf, bkg, kw, ks):
    """Run the reference; returns {k: locals at the head of iteration k} for
    every k in ks and k + 1, and {k: line-search trials of iteration k}."""
    want = set(ks) | {k + 1 for k in ks}
    snaps, trials = {}, {}
    code = getattr(sgp, fn).__code__

    def local(frame, event, arg):
        if event != "line":
            return local
        src = linecache.getline(code.co_filename, frame.f_lineno).strip()
        if src == "prev_x = x.copy()":
            L = frame.f_locals
            it = int(L["iter_"])
            if it in want:
                s = {v: np.array(L[v], dtype=np.float64).copy() for v in VECS + ("gn", "bkg")}
                s.update({v: float(L[v]) for v in SCALARS})
                s["Valpha"] = np.array(L["Valpha"], dtype=np.float64).copy()
                s["Fold"] = np.array(L["Fold"], dtype=np.float64).copy()
                s["tol"] = float(L["tol"]) if np.isscalar(L["tol"]) else 0.0
                s["iter_"] = it
                if fn == "sgp_betaDiv":
                    s.update(betaParam=float(L["betaParam"]), lr=float(L["lr"]),
                             epoch=int(L["epoch"]))
                snaps[it] = s
        elif src.startswith("if fv <= fr + gamma * lam * gd"):
            it = int(frame.f_locals["iter_"])
            trials[it] = trials.get(it, 0) + 1
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None

    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())  # the reference writes sgp.log to the cwd
    sys.settrace(tracer)
    try:
        getattr(sgp, fn)(gn.copy(), psf, np.float64(bkg), MAXIT=max(ks) + 1, **kw)
    finally:
        sys.settrace(None)
        os.chdir(cwd)
    return snaps, trials


def main():
    sgp, _ = import_reference(need_astropy=False)
    # seed 3: in the reference the beta run's iteration 150 backtracks once (2
    # trials) without stagnating.  (Seed 17 stagnates there, 24 trials: its
    # accepted step is 1e-9 of d, the Barzilai-Borwein sums are then
    # differences at the rounding level and no 1e-9 check of alpha.)
    gn, _, _ = synth_field(64, 64, 40, seed=3, bkg=100.0)
    psf = gaussian_psf(64, fwhm=5.0)
    out = dict(psf=psf, gn_raw=gn, bkg_raw=np.float64(100.0),
               cases=np.array(sorted(CASES)))
    for name, (fn, kw, ks) in CASES.items():
        snaps, trials = capture(sgp, fn, gn, psf, 100.0, kw, ks)
        out[f"{name}_fn"], out[f"{name}_kwargs"] = np.array(fn), np.array(repr(kw))
        out[f"{name}_ks"] = np.array(ks)
        out[f"{name}_gn"] = snaps[ks[0]]["gn"].reshape(64, 64)
        for k in ks:
            s, n = snaps[k], snaps[k + 1]
            assert s["iter_"] == k and n["iter_"] == k + 1
            assert np.array_equal(s["gn"], snaps[ks[0]]["gn"]) and s["bkg"].size == 1
            p = f"{name}_k{k}_"
            for v in VECS:
                out[p + v] = s[v].reshape(64, 64)
            out[p + "x_next"] = n["x"].reshape(64, 64)
            keys = SCALARS + (("betaParam", "lr") if fn == "sgp_betaDiv" else ())
            out[p + "scalars"] = np.array([s[v] for v in keys])
            out[p + "next"] = np.array([n[v] for v in keys])
            out[p + "names"] = np.array(keys)
            out[p + "Valpha"], out[p + "Fold"] = s["Valpha"], s["Fold"]
            out[p + "tol"], out[p + "bkg"] = np.float64(s["tol"]), np.float64(s["bkg"][0])
            out[p + "trials"] = np.int64(trials[k])
            if fn == "sgp_betaDiv":
                assert s["epoch"] == k  # incremented before the loop head line
            print(f"{name:6s} k={k:3d} trials={trials[k]} fv={s['fv']:.15g} -> {n['fv']:.15g} "
                  f"alpha={s['alpha']:.6g} -> {n['alpha']:.6g}")
    path = os.path.join(HERE, "ref_states.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
