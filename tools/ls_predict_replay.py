"""How well does "this line search ends like the previous one" predict?

The evidence for the line-search predictor of ls_phase (bsgp_kernels.hpp,
SolveArgs::ls_predict): the numpy oracle solves bench-generator stamps (C3
parameters) on the CPU, its per-iteration trial counts (stats['ls_trials'])
become outcome strings, and the rule the kernel applies to the last accepted
step is replayed on them.

    python tools/ls_predict_replay.py [--images 4] [--maxit 100] [--seed0 10000]

An iteration that accepts after n trials took the step lam = beta^(n-1)
(beta: the backtracking factor, 0.4).  Its outcome is
    A   n == 1: the first trial, lam = 1, is accepted;
    S   lam < threshold: the search stagnates (many trials, all but the first
        from the closed-form series);
    M   anything between.
The rule predicts A after an A, S after an S and nothing after an M; a
prediction is a hit when the iteration ends as predicted.  (The kernel's
default uses the A half only: the S half measured slower)
CPU only.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BACKTRACK = 0.4       # solve_kwargs' beta (sgp.DEFAULT_PARAMS)
STAG_LAM = 1e-4       # kLsStagLam of ls_phase


def step_of(trials, backtrack=BACKTRACK):
    """The accepted step of a search that took `trials` trials: the sequential
    products lam *= beta of the solver, so the same float64 value."""
    lam = 1.0
    for _ in range(int(trials) - 1):
        lam = lam * backtrack
    return lam


def outcome(trials, stag_lam=STAG_LAM, backtrack=BACKTRACK):
    lam = step_of(trials, backtrack)
    return "A" if lam == 1.0 else ("S" if lam < stag_lam else "M")


def outcomes(ls_trials, stag_lam=STAG_LAM, backtrack=BACKTRACK):
    """Outcome string of one image, one letter per iteration."""
    return "".join(outcome(n, stag_lam, backtrack) for n in ls_trials)


def predict(prev_lam, stag_lam=STAG_LAM):
    """ls_phase's rule on the last accepted step (the setup leaves 1.0)."""
    return "A" if prev_lam == 1.0 else ("S" if prev_lam < stag_lam else "-")


def score(s):
    """Replay the predictor on an outcome string.  Returns a dict: iterations,
    predictions made per kind, hits per kind, and the hit rate over all
    iterations (an iteration without a prediction counts as no hit)."""
    r = dict(n=len(s), pred_A=0, pred_S=0, none=0, hit_A=0, hit_S=0)
    prev = "A"  # st.lam = 1 after the setup
    for c in s:
        p = prev if prev in "AS" else "-"
        if p == "-":
            r["none"] += 1
        else:
            r["pred_" + p] += 1
            r["hit_" + p] += p == c
        prev = c
    r["hit_rate"] = (r["hit_A"] + r["hit_S"]) / r["n"] if r["n"] else 0.0
    return r


def solve_trials(seed, maxit, n=256, k=25, nstars=200):
    """ls_trials of one bench-generator image under the oracle (C3 parameters)."""
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np

    import cpu_bench
    import sgp_oracle
    gn, psf = cpu_bench.make_stamp(seed, n, k, nstars, circular=False)
    kw = dict(init_recon=2, proj_type=1, stop_criterion=1, MAXIT=maxit, tol_convergence=1e-5,
              gamma=1e-4, beta=BACKTRACK, alpha=10.0, alpha_min=1e-5, alpha_max=1e5, M_alpha=3,
              tau=0.5, M=1, max_projs=1000, ccd_sat_level=65000.0, scale_data=True,
              use_original_SGP_Afunction=False, adapt_beta=False, betaParam=1.05, lr=1e-3,
              lr_exp_param=0.1, schedule_lr=True, verbose=False)
    stats = {}
    sgp_oracle.sgp_betaDiv(gn, psf, np.float64(100.0), stats=stats, **kw)
    return list(stats["ls_trials"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--seed0", type=int, default=10000)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--thresholds", default="1e-2,1e-4,1e-6",
                    help="stagnation thresholds on the last step to compare")
    args = ap.parse_args()
    trials = []
    for i in range(args.images):
        t = solve_trials(args.seed0 + i, args.maxit, n=args.n)
        trials.append(t)
        s = outcomes(t)
        sw = next((j for j, c in enumerate(s) if c != "A"), len(s))
        print(f"seed {args.seed0 + i}: first non-accept at iteration {sw + 1}\n  {s}")
        print("  trials: " + " ".join(str(n) for n in t))
    for th in (float(x) for x in args.thresholds.split(",")):
        tot = dict(n=0, pred_A=0, pred_S=0, none=0, hit_A=0, hit_S=0)
        for t in trials:
            r = score(outcomes(t, th))
            for key in tot:
                tot[key] += r[key]
        n = tot["n"]
        print(f"threshold {th:g}: {n} iterations; predicted accept {tot['pred_A'] / n:.1%} "
              f"(hits {tot['hit_A']}/{tot['pred_A']}), predicted stagnation "
              f"{tot['pred_S'] / n:.1%} (hits {tot['hit_S']}/{tot['pred_S']}), no prediction "
              f"{tot['none'] / n:.1%}; hit rate over all iterations "
              f"{(tot['hit_A'] + tot['hit_S']) / n:.1%}")


if __name__ == "__main__":
    main()
