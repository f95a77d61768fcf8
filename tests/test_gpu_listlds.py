"""Projection pixel lists of one-workgroup images in the transform buffers' LDS
(cached_projection, SolveArgs::list_lds; BSGP_LIST_LDS caps the entries per
thread, 0 keeps every entry in global memory).  Where an entry lives changes
neither its value nor the order a thread sums its list in, so every cap gives
the same bits, in the persistent solver and in the phase kernels: caps 1 and 2
send every thread with a longer list through the LDS / global split, the
default keeps as many entries as the buffers hold.  MI355X tests.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

KEYS = ("x", "iters", "discr", "flags", "beta_final", "counters")

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


def case(shape):
    if shape == "40x70":
        fx = golden("ref_c3stop3_s0.npz")
        g = fx["gn"].astype(np.float64)
        gns = np.stack([g[100:140, 60:130], g[20:60, 150:220], g[200:240, 10:80],
                        g[150:190, 100:170]])
        return gns, fx["psf"], np.full(4, 100.0), dict(C3_KW, MAXIT=30,
                                                       betaParams=[1.05, 0.97, 1.02, 1.08])
    if shape == "64x64":
        fx = golden("ref_lin64_beta.npz")
        g = fx["gn"].astype(np.float64)
        gns = np.stack([np.roll(g, 5 * i, 1) for i in range(4)])
        return gns, fx["psf"], np.full(4, 100.0), dict(C3_KW, MAXIT=30,
                                                       betaParams=[1.05, 0.97, 1.02, 0.99])
    import cpu_bench  # one image of the timed workload (the static 270-point plan)
    gn, psf = cpu_bench.make_stamp(10000, 256, 25, 200)[:2]
    return gn[None], psf, np.full(1, 100.0), dict(C3_KW, MAXIT=25, betaParams=1.05)


@pytest.mark.parametrize("shape", ["64x64", "40x70", "256x256"])
def test_every_cap_gives_the_same_bits(sgpmod, monkeypatch, shape):
    gns, psf, bkg, kw = case(shape)
    base = None
    for cap in ("0", "1", "2", None):
        if cap is None:
            monkeypatch.delenv("BSGP_LIST_LDS", raising=False)
        else:
            monkeypatch.setenv("BSGP_LIST_LDS", cap)
        for persistent in (1, 0):
            out = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=persistent, proj_cache=1, **kw)
            assert np.all(out["counters"][:, 3] == 0)
            if base is None:
                base = out
                continue
            for k in KEYS:
                np.testing.assert_array_equal(
                    out[k], base[k], err_msg=f"{k}: BSGP_LIST_LDS={cap}, persistent={persistent}")
    # counters[:, 7]: list entries read by the projections' list evaluations
    assert np.all(base["counters"][:, 7] > 0), base["counters"]
