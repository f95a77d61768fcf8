"""The persistent solver's compile-time-geometry path (SGeo256, k_persist's
static phase functions): 256 x 256 images on the 270 x 270 grid of
a 25 x 25 PSF in linear mode, float64 storage, general fixed beta, one
workgroup per image.  The path folds the plan's geometry into constants and
changes no arithmetic, so a solve on it equals the runtime-geometry solve and
the phase kernels bit for bit: x, discr, iters, beta_final, the per-iteration
flags / trial counts and every device counter.  ``static_geo=0/1`` of the batch
functions chooses per solve; ``sgp.last_static_geo()`` reports what ran.  Plans
that differ from the static geometry in any value take the runtime path
whatever the knob says.  MI355X tests.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("x", "iters", "discr", "flags", "beta_final", "counters")
SEEDS = tuple(range(10000, 10006))  # bench-generator seeds (oracle/cpu_bench.make_stamp)

C3_KW = dict(init_recon=2, proj_type=1, stop_criterion=1, tol_convergence=1e-5, gamma=1e-4,
             beta=0.4, alpha=10.0, alpha_min=1e-5, alpha_max=1e5, M_alpha=3, tau=0.5, M=1,
             max_projs=1000, ccd_sat_level=65000.0, scale_data=True,
             use_original_SGP_Afunction=False, adapt_beta=False, lr=1e-3, lr_exp_param=0.1,
             schedule_lr=True, team=1, betaParams=1.05)


@pytest.fixture(scope="module")
def sgpmod():
    import _bsgp
    _bsgp.require_gpu()
    import sgp
    return sgp


@pytest.fixture(scope="module")
def stamps():
    """(images [6, 256, 256] float64, the 25 x 25 PSF): C3's generator."""
    import cpu_bench
    st = [cpu_bench.make_stamp(s, 256, 25, 200) for s in SEEDS]
    return np.stack([s[0] for s in st]).astype(np.float64), st[0][1]


def same(a, b, what):
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{k}: {what}")


def three_ways(sgpmod, fn, gns, psf, bkg, kw):
    """static path, runtime path, phase kernels: the same bits; returns the first."""
    on = fn(gns, psf, bkg, persistent=1, static_geo=1, **kw)
    assert sgpmod.last_static_geo(), "the static path did not run"
    off = fn(gns, psf, bkg, persistent=1, static_geo=0, **kw)
    assert not sgpmod.last_static_geo()
    ph = fn(gns, psf, bkg, persistent=0, static_geo=1, **kw)
    assert not sgpmod.last_static_geo(), "phase kernels have no static path"
    assert np.all(on["counters"][:, 3] == 0)
    same(off, on, "static_geo=0 against 1")
    same(ph, on, "persistent=0 against the static path")
    return on


def test_main_path_equals_runtime_path_and_phase_kernels(sgpmod, stamps):
    """Six C3 images, scalar background, MAXIT 60: predicted accepts, failed
    predictions with their replay, second trials from pass 1, direct passes and
    closed-form stagnation all occur (the searches leave lam = 1 between
    iterations 9 and 56 and stagnate from about 30 on)."""
    gns, psf = stamps
    out = three_ways(sgpmod, sgpmod.sgp_betaDiv_batch, gns, psf, np.full(len(gns), 100.0),
                     dict(C3_KW, MAXIT=60))
    t = ((np.asarray(out["flags"]) >> 8) & 0xffff)[:, 1:61]
    assert (out["iters"] == 60).all()
    print("trials per iteration:", t.tolist(), "ls passes:", out["counters"][:, 2].tolist(),
          "closed-form trials:", out["counters"][:, 4].tolist())
    assert (t[:, :5] == 1).all() and (t >= 2).any() and (t >= 16).any(), t
    assert (out["counters"][:, 4] > 0).any()  # closed-form trials ran


def test_background_map_path(sgpmod, stamps):
    """The build with the per-pixel background operand (SB = false)."""
    gns, psf = stamps
    yy, xx = np.mgrid[0:256, 0:256]
    ramp = 100.0 * (1.0 + 0.05 * np.sin(0.37 * yy + 0.1) * np.cos(0.23 * xx))
    three_ways(sgpmod, sgpmod.sgp_betaDiv_batch, gns[:3], psf, np.broadcast_to(ramp, (3, 256, 256)),
               dict(C3_KW, MAXIT=25))


def test_float32_image_path(sgpmod, stamps):
    """The same counts as float32 images (MODE 4: the objective's
    float32-rounded factors, numpy's float32 sum order on the one-workgroup
    team) run k_persist<false, 2, 4, false, double>'s static phases."""
    gns, psf = stamps
    g32 = gns[:3].astype(np.float32)
    assert np.array_equal(g32.astype(np.float64), gns[:3])
    three_ways(sgpmod, sgpmod.sgp_betaDiv_batch, g32, psf, np.full(3, 100.0),
               dict(C3_KW, MAXIT=25))


def test_more_images_than_slots(sgpmod, stamps):
    """772 images (more than 256 CUs x 3 workgroups), MAXIT 3: every slot of
    the static path's queue is reused; eight of the images solved alone on the
    runtime path give the same bits."""
    import torch
    gns, psf = stamps
    base = torch.from_numpy(gns).cuda()
    B = 772
    batch = torch.stack([torch.roll(base[i % 6], shifts=(3 * (i // 6), 5 * (i // 6)), dims=(0, 1))
                         for i in range(B)])
    kw = dict(C3_KW, MAXIT=3)
    bkg = torch.full((B,), 100.0, dtype=torch.float64, device="cuda")
    out = sgpmod.sgp_betaDiv_batch(batch, psf, bkg, persistent=1, static_geo=1, device_out=True,
                                   **kw)
    assert sgpmod.last_static_geo()
    idx = [0, 1, 255, 256, 511, 767, 768, 771]
    alone = sgpmod.sgp_betaDiv_batch(batch[idx], psf, bkg[idx], persistent=1, static_geo=0,
                                     device_out=True, **kw)
    assert not sgpmod.last_static_geo()
    torch.cuda.synchronize()
    assert (out["iters"].cpu().numpy() == 3).all()
    for k in KEYS:
        np.testing.assert_array_equal(out[k][idx].cpu().numpy(), alone[k].cpu().numpy(), err_msg=k)


def gauss_psf(k, sigma):
    a = np.arange(k) - k // 2
    g = np.exp(-0.5 * (a / sigma) ** 2)
    p = np.outer(g, g)
    return p / p.sum()


@pytest.mark.parametrize("shape", ["circular", "255x256", "psf31", "f32", "kl"])
def test_other_plans_take_the_runtime_path(sgpmod, stamps, shape):
    """Anything but the static plan reports the runtime path with the knob on,
    and gives the same bits with it on and off.  The KL objective has no static
    build (the static phases exist for the general-beta kernels)."""
    gns, psf = stamps
    gns = gns[:2]
    kw = dict(C3_KW, MAXIT=5)
    fn = sgpmod.sgp_betaDiv_batch
    if shape == "circular":
        import cpu_bench
        kw["use_original_SGP_Afunction"] = True  # P = Q = 256; the PSF as a full-size image
        psf = cpu_bench.embed_psf(psf, 256)
    elif shape == "255x256":
        gns = np.ascontiguousarray(gns[:, :255, :])
    elif shape == "psf31":
        psf = gauss_psf(31, 2.5)  # 256 + 15 -> a 272-point grid
    elif shape == "f32":
        kw["storage"] = "f32"
    else:
        fn = sgpmod.sgp_batch
        kw = {k: v for k, v in kw.items()
              if k not in ("betaParams", "adapt_beta", "lr", "lr_exp_param", "schedule_lr")}
    bkg = np.full(2, 100.0)
    on = fn(gns, psf, bkg, persistent=1, static_geo=1, **kw)
    assert not sgpmod.last_static_geo(), f"{shape}: took the static path"
    off = fn(gns, psf, bkg, persistent=1, static_geo=0, **kw)
    assert not sgpmod.last_static_geo()
    same(off, on, shape)


def test_saved_and_resumed_on_the_static_path(sgpmod, stamps):
    """A static-path solve saved at iteration 20 and resumed to 40 (again on
    the static path) equals the uninterrupted solve."""
    gns, psf = stamps
    gns = gns[:3]
    bkg = np.full(3, 100.0)
    whole = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=1, static_geo=1,
                                     **dict(C3_KW, MAXIT=40))
    assert sgpmod.last_static_geo()
    first = sgpmod.sgp_betaDiv_batch(gns, psf, bkg, persistent=1, static_geo=1, return_state=True,
                                     **dict(C3_KW, MAXIT=20))
    assert sgpmod.last_static_geo()
    part = sgpmod.sgp_resume(first["state"], 40, persistent=1, static_geo=1)
    assert sgpmod.last_static_geo(), "the resumed solve left the static path"
    for k in KEYS:
        assert part[k].shape == whole[k].shape, k  # both histories have MAXIT 40's rows
        np.testing.assert_array_equal(part[k], whole[k], err_msg=k)


def test_a_failed_solve_consumes_the_choice(sgpmod, stamps, monkeypatch):
    """bsgp_plan_set_static_geo holds for the next solve only: a solve that
    fails its argument checks uses the choice up and reports no static path,
    and the solve after it takes the default again."""
    import torch
    import _bsgp
    monkeypatch.setenv("BSGP_STATIC_GEO", "1")
    gns, psf = stamps
    kw = {k: v for k, v in dict(C3_KW, MAXIT=3, persistent=1).items()
          if k != "use_original_SGP_Afunction"}
    good = sgpmod.state_params("beta", **kw)
    bad = sgpmod.state_params("beta", **dict(kw, M_alpha=99))  # refused by the library
    gd = torch.from_numpy(gns[:2]).cuda()
    bd = torch.full((2,), 100.0, dtype=torch.float64, device="cuda")
    b0 = torch.full((2,), 1.05, dtype=torch.float64, device="cuda")
    with _bsgp.lease_plan(256, 256, psf, _bsgp.BSGP_CONV_LINEAR_FILL) as plan:
        plan.solve(gd, bd, good, beta0=b0)
        assert plan.static_geo_used()
        plan.set_static_geo(0)
        with pytest.raises(_bsgp.BsgpError):
            plan.solve(gd, bd, bad, beta0=b0)
        assert not plan.static_geo_used()
        out = plan.solve(gd, bd, good, beta0=b0)
        assert plan.static_geo_used(), "the failed solve's static_geo=0 leaked into this one"
        torch.cuda.synchronize()
        assert (out["iters"].cpu().numpy() == 3).all()
