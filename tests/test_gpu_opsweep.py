"""A / AT on the device against the exact reference (tests/op_ref.py) at one
shape per branch of plan_layout, then the batch paths, per-image PSFs and short
solves at the odd ones.  All tests need an MI355X.

The table is op_ref.SWEEP; tests/test_op_ref.py holds every row to its branch
on the host.  The tolerance of a case is op_ref.FACTOR (8) times what numpy's
own float64 FFT operator misses the exact reference by, in that case, image,
direction and norm (relative L2 and max|out - ref| / max|ref|), and never above
the earlier bar of the suite (1e-13 in L2; 1e-12 in max-norm): a margin over
the reference's error, not over the device's.  No case takes more than 8.

With BSGP_OPSWEEP_RECORD=<file> every comparison appends its figures (device,
numpy, ratio) to that file: profiles/opsweep/errors.txt is one such run.
"""
import os

import numpy as np
import pytest

import op_ref
from op_ref import BATCH, BY_ID, CIRC, PER_IMAGE, SOLVE, SWEEP

pytestmark = pytest.mark.gpu

SOLVE_RTOL = 1e-5  # tests/test_gpu_parity.py


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


def _record(what, l2, mx, nl2, nmx):
    line = (f"{what}: L2 device {l2:.3e} numpy {nl2:.3e} ratio {l2 / max(nl2, 1e-300):.2f}; "
            f"max device {mx:.3e} numpy {nmx:.3e} ratio {mx / max(nmx, 1e-300):.2f}")
    print(line)
    path = os.environ.get("BSGP_OPSWEEP_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def check_against_exact(what, out, x, psf, mode, tr):
    """Every image of `out` (the device's A or AT of x) within the case's
    tolerance of the exact reference."""
    ref = op_ref.op_ref(x, psf, mode, tr)
    ours = op_ref.numpy_op(x, psf, mode, tr)
    for i in range(len(x)):
        l2, mx = op_ref.errors(out[i], ref[i])
        nl2, nmx = op_ref.errors(ours[i], ref[i])
        tl2, tmx = op_ref.tolerances(nl2, nmx)
        _record(f"{what} {'AT' if tr else 'A'} image {i}", l2, mx, nl2, nmx)
        assert l2 <= tl2 and mx <= tmx, (what, tr, i, (l2, tl2), (mx, tmx))


def slots_of(case):
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return ncu * case.layout()["wg_per_cu"]


# ------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c.id)
def test_operator_matches_exact_reference(B, case):
    assert op_ref.misplaced(case) == {}
    psf, x = case.psf(), case.images()
    plan = B.Plan(case.H, case.W, psf, case.mode)
    for tr in (False, True):
        out = plan.apply(B.to_dev(x), transpose=tr).cpu().numpy()
        # nothing of a neighbouring slot or an earlier spectrum in the zero image
        assert not out[2].any(), (tr, np.abs(out[2]).max())
        check_against_exact(case.id, out[:2], x[:2], psf, case.mode, tr)


# ---------------------------------------------------------------- batch paths
@pytest.mark.parametrize("many", [False, True], ids=["persistent", "several-per-workgroup"])
@pytest.mark.parametrize("cid", BATCH)
def test_batch_paths_are_the_single_image_call(B, cid, many):
    """One workgroup per image (B * 4 > slots) and several images per
    workgroup (B > slots: apply_op_kernel's image loop): every image has the
    bits of its own single-image call, which spreads it over many workgroups."""
    import torch
    case = BY_ID[cid]
    slots = slots_of(case)
    n = slots + 5 if many else slots // 4 + 1
    rng = np.random.default_rng(case.seed() + [3, n])
    x = rng.uniform(0, 1, (n, case.H, case.W))
    x[:, 0, 0] = 50.0
    x[:, -1, -1] = 80.0
    psf = case.psf()
    plan = B.Plan(case.H, case.W, psf, case.mode)
    xd = B.to_dev(x)
    idx = sorted({i for i in (0, slots - 1, slots, n - 1) if i < n})
    for tr in (False, True):
        batch = plan.apply(xd, transpose=tr)
        singles = torch.stack([plan.apply(xd[i:i + 1], transpose=tr)[0] for i in range(n)])
        diff = (batch != singles).flatten(1).any(1).nonzero().flatten().tolist()
        assert not diff, (tr, n, diff[:20])
        check_against_exact(f"{cid} B={n} images {idx}", batch[idx].cpu().numpy(), x[idx], psf,
                            case.mode, tr)


# ------------------------------------------------------------- per-image PSFs
@pytest.mark.parametrize("cid", PER_IMAGE)
def test_per_image_psfs(B, cid):
    """bsgp_plan_set_psfs: image i takes PSF i, with the bits of a plan made
    from that PSF alone (place_psfs_kernel places what the host places)."""
    case = BY_ID[cid]
    n = 5
    psfs = np.stack([case.psf(variant=v + 1) for v in range(n)])
    x = np.stack([case.images(variant=v + 1)[0] for v in range(n)])
    plan = B.Plan(case.H, case.W, psfs[0], case.mode).set_psfs(B.to_dev(psfs))
    own = [B.Plan(case.H, case.W, psfs[i], case.mode) for i in range(n)]
    for tr in (False, True):
        out = plan.apply(B.to_dev(x), transpose=tr).cpu().numpy()
        for i in range(n):
            one = own[i].apply(B.to_dev(x[i:i + 1]), transpose=tr).cpu().numpy()[0]
            np.testing.assert_array_equal(out[i], one)
            check_against_exact(f"{cid} psf {i}", out[i:i + 1], x[i:i + 1], psfs[i], case.mode, tr)


# --------------------------------------------------------------- short solves
# test_c4_field_2048_matches_oracle's keywords, four iterations
KW = dict(init_recon=2, proj_type=1, stop_criterion=1, MAXIT=4, alpha=10.0, ccd_sat_level=65000.0)
BETA_KW = dict(schedule_lr=True, adapt_beta=False)

_FIELDS = {}


def star_field(case, variant=0):
    """A few stars through the case's PSF, background 100, Poisson noise."""
    key = (case.id, variant)
    if key not in _FIELDS:
        rng = np.random.default_rng(case.seed() + [4, variant])
        psf = case.psf()
        obj = np.zeros((case.H, case.W))
        for _ in range(6):
            obj[rng.integers(case.H), rng.integers(case.W)] += rng.uniform(2000.0, 8000.0)
        mean = op_ref.numpy_op(obj[None], psf, case.mode)[0]
        gn = rng.poisson(np.maximum(mean, 0.0) + 100.0).astype(np.float64)
        _FIELDS[key] = (gn, psf)
    return _FIELDS[key]


@pytest.mark.parametrize("fn", ["sgp", "sgp_betaDiv"])
@pytest.mark.parametrize("cid", SOLVE)
def test_short_solve_matches_oracle(sgpmod, cid, fn):
    """Four iterations at the odd shapes: the solver's own instantiations of
    the row passes (pipelined, prefetching, wide loads, the 512-thread build)."""
    import sgp_oracle
    case = BY_ID[cid]
    gn, psf = star_field(case)
    kw = dict(KW, use_original_SGP_Afunction=case.mode == CIRC)
    if fn == "sgp_betaDiv":
        kw.update(BETA_KW, betaParam=1.05)
    xr, itr, dr, _, _ = getattr(sgp_oracle, fn)(gn, psf, np.float64(100.0), **kw)
    x, it, d, _, _ = getattr(sgpmod, fn)(gn, psf, np.float64(100.0), **kw)
    assert it == itr
    assert rel(x, xr) < SOLVE_RTOL, rel(x, xr)
    np.testing.assert_allclose(d, dr, rtol=1e-7)


def test_short_solve_f32_storage(sgpmod):
    """45 x 50, 5 x 3 kernel, iteration vectors in float32: the suite's 1e-3."""
    import sgp_oracle
    case = BY_ID["45x50-lin-k5x3"]
    gn, psf = star_field(case)
    kw = dict(KW, use_original_SGP_Afunction=False, **BETA_KW)
    xr, itr, dr, _, _ = sgp_oracle.sgp_betaDiv(gn, psf, np.float64(100.0), betaParam=1.05, **kw)
    out = sgpmod.sgp_betaDiv_batch(gn[None], psf, 100.0, storage="f32", betaParams=1.05, **kw)
    assert int(out["iters"][0]) == itr
    assert rel(out["x"][0], xr) < 1e-3, rel(out["x"][0], xr)
    np.testing.assert_allclose(out["discr"][0, :itr + 1], dr, rtol=1e-3)


@pytest.mark.parametrize("cid", ["33x31-lin-k6x8", "8x600-circ"])
def test_short_solve_batch_is_bitwise_the_single_solves(sgpmod, cid):
    case = BY_ID[cid]
    gns = np.stack([star_field(case, v)[0] for v in range(3)])
    psf = case.psf()
    kw = dict(KW, use_original_SGP_Afunction=case.mode == CIRC, team=1, **BETA_KW)
    betas = [1.05, 0.97, 1.02]
    out = sgpmod.sgp_betaDiv_batch(gns, psf, 100.0, betaParams=betas, **kw)
    assert np.all(out["counters"][:, 5] == 1)
    for i in range(3):
        one = sgpmod.sgp_betaDiv_batch(gns[i:i + 1], psf, 100.0, betaParams=betas[i:i + 1], **kw)
        assert one["iters"][0] == out["iters"][i]
        np.testing.assert_array_equal(one["x"][0], out["x"][i])
        np.testing.assert_array_equal(one["discr"][0], out["discr"][i])
