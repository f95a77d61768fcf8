"""Solver-state records on the host (no GPU): SolverState.from_arrays builds
records from plain arrays, save / load is an identity on every field, a wrong
layout version or shape is refused, and the new C entry points validate their
arguments without a device."""
import ctypes

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)


def _state(bmap=False, storage="f64", Bn=2, H=7, W=9, done=4):
    import _bsgp
    import sgp
    rng = np.random.default_rng(3)
    prm = sgp._params(_bsgp.BSGP_VARIANT_BETA, 2, 1, 3, 20, 1e-4, 0.4, 1.3, 1e-5, 1e5, 3, 0.5, 2,
                      1000, False, 60000.0, True, 1e-4, betaParam=1.05, lr=2e-3)
    psf = np.full((H, W), 1.0 / (H * W))
    v = {k: rng.random((Bn, H, W)) for k in ("x", "g", "x_tf", "gn", "pw")}
    bkg = rng.random((Bn, H, W)) if bmap else rng.random(Bn)
    sc = dict(iters_done=done, alpha=rng.random(Bn), tau=0.45, fv=rng.random(Bn),
              flux=rng.random(Bn), scaling=[3.0, 5.0], x_low=1e-3, x_upp=[7.0, 9.0], tol=1e-4,
              Valpha=rng.random((Bn, 3)), Fold=rng.random((Bn, 2)), beta=[1.04, 1.06],
              lr=1.5e-3, konst=rng.random(Bn), lam_p=rng.random(Bn), lam_ratio=0.25, kappa=1.9,
              elapsed=0.125, counters=rng.integers(0, 1000, (Bn, 7)),
              discr=rng.random((Bn, done + 1)), crit=rng.random((Bn, done + 1)),
              times=rng.random((Bn, done + 1)), flags=rng.integers(0, 999, (Bn, done + 1)),
              team=2, storage=storage, conv_mode=_bsgp.BSGP_CONV_CIRCULAR, stopped=[0, 1])
    st = _bsgp.SolverState.from_arrays(psf, prm, v["x"], v["g"], v["x_tf"], v["gn"], pw=v["pw"],
                                       bkg=bkg, **sc)
    return st, v, bkg, sc, prm


@pytest.mark.parametrize("bmap,storage", [(False, "f64"), (True, "f64"), (False, "f32")])
def test_from_arrays_save_load_is_identity(tmp_path, bmap, storage):
    import _bsgp
    st, v, bkg, sc, prm = _state(bmap, storage)
    vdt = np.float32 if storage == "f32" else np.float64
    # what went in is what the documented fields hold
    for k in ("x", "g", "x_tf", "pw"):
        np.testing.assert_array_equal(st.field(k), v[k].astype(vdt))
    np.testing.assert_array_equal(st.field("gn"), v["gn"])
    h = st.header
    assert h.dtype.itemsize <= _bsgp.BSGP_STATE_HEADER_BYTES
    if bmap:
        np.testing.assert_array_equal(st.field("bkg"), bkg)
    else:
        assert st.field("bkg") is None
        np.testing.assert_array_equal(h["bkg_scalar"], bkg)
    for k in ("discr", "crit", "times", "flags"):
        np.testing.assert_array_equal(st.field(k), sc[k])
    for k in ("alpha", "fv", "flux", "konst", "lam_p"):
        np.testing.assert_array_equal(h[k], sc[k])
    np.testing.assert_array_equal(h["scaling"], [3.0, 5.0])
    np.testing.assert_array_equal(h["Dcoeff"], 2 / 63.0 * np.array([3.0, 5.0]))
    np.testing.assert_array_equal(h["Valpha"][:, :3], sc["Valpha"])
    np.testing.assert_array_equal(h["Valpha"][:, 3:], 0.0)
    np.testing.assert_array_equal(h["Fold"][:, :2], sc["Fold"])
    np.testing.assert_array_equal(h["counters"], sc["counters"])
    np.testing.assert_array_equal(h["beta"], [1.04, 1.06])
    assert list(h["T"]) == [2, 2] and list(h["epoch"]) == [4, 4]
    np.testing.assert_array_equal(st.iters_done, [4, 4])
    np.testing.assert_array_equal(st.stopped, [False, True])
    q = st.params()
    assert q.MAXIT == 20 and q.gamma == prm.gamma
    assert q.bkg_is_map == int(bmap) and q.betaParam == 1.05 and q.has_sat == 1
    # disk round trip: every byte of every record, and the PSF
    path = str(tmp_path / "state.npz")
    st.save(path)
    back = _bsgp.SolverState.load(path)
    assert back.records.dtype == np.uint8 and back.records.shape == st.records.shape
    np.testing.assert_array_equal(back.records, st.records)
    np.testing.assert_array_equal(back.psf, st.psf)
    for name in h.dtype.names:
        if name != "prm":
            np.testing.assert_array_equal(back.header[name], h[name])
    assert back.header["prm"].tobytes() == h["prm"].tobytes()
    # subset selection keeps whole records
    sub = back[[1, 0]]
    np.testing.assert_array_equal(sub.records, st.records[[1, 0]])
    np.testing.assert_array_equal(sub.stopped, [True, False])
    assert len(back[1]) == 1 and back[1].header["scaling"][0] == 5.0


def test_record_layout_is_the_documented_one():
    """16-byte aligned sections in the header's order, N elements each, the
    plan's padding removed (include/bsgp.h)."""
    import _bsgp
    L = _bsgp.state_layout(31, 31, _bsgp.BSGP_STORAGE_F64, False, 13)
    N = 961
    pad = lambda n: (n + 15) // 16 * 16  # noqa: E731
    assert L["discr"] == _bsgp.BSGP_STATE_HEADER_BYTES
    assert L["crit"] - L["discr"] == pad(13 * 8) and L["flags"] - L["times"] == pad(13 * 8)
    assert L["x"] - L["flags"] == pad(13 * 4)
    assert L["g"] - L["x"] == pad(N * 8) == L["gn"] - L["pw"]
    assert L["bkg"] == 0 and L["bytes"] == L["gn"] + pad(N * 8)
    assert all(v % 16 == 0 for v in L.values())
    L32 = _bsgp.state_layout(31, 31, _bsgp.BSGP_STORAGE_F32, True, 13)
    assert L32["g"] - L32["x"] == pad(N * 4) and L32["bkg"] - L32["gn"] == pad(N * 8)
    assert L32["bytes"] == L32["bkg"] + pad(N * 8)
    # the issue's size estimate: 256^2 f64 with a scalar background, 5 x 512 KiB
    big = _bsgp.state_layout(256, 256, 0, False, 101)["bytes"]
    assert 5 * 512 * 1024 < big < 5 * 512 * 1024 + 8192


def test_load_refuses_wrong_version_or_shape(tmp_path):
    import _bsgp
    st, *_ = _state()
    path = str(tmp_path / "s.npz")
    st.save(path)
    with np.load(path) as z:
        d = {k: z[k] for k in z.files}
    bad = dict(d, version=np.int64(_bsgp.BSGP_STATE_VERSION + 1))
    np.savez(str(tmp_path / "v.npz"), **bad)
    with pytest.raises(ValueError, match="version"):
        _bsgp.SolverState.load(str(tmp_path / "v.npz"))
    rec = d["records"].copy()
    rec[:, 4:8] = np.frombuffer(np.uint32(7).tobytes(), np.uint8)  # header.version
    np.savez(str(tmp_path / "v2.npz"), **dict(d, records=rec))
    with pytest.raises(ValueError, match="version"):
        _bsgp.SolverState.load(str(tmp_path / "v2.npz"))
    np.savez(str(tmp_path / "s2.npz"), **dict(d, shape=np.asarray([9, 7], np.int64)))
    with pytest.raises(ValueError, match="shape"):
        _bsgp.SolverState.load(str(tmp_path / "s2.npz"))
    rec = d["records"].copy()
    rec[1, 8:12] = np.frombuffer(np.int32(8).tobytes(), np.uint8)  # header.H of record 1
    np.savez(str(tmp_path / "s3.npz"), **dict(d, records=rec))
    with pytest.raises(ValueError, match="shape"):
        _bsgp.SolverState.load(str(tmp_path / "s3.npz"))
    rec = d["records"].copy()
    rec[0, 0] ^= 0xFF
    np.savez(str(tmp_path / "m.npz"), **dict(d, records=rec))
    with pytest.raises(ValueError, match="magic"):
        _bsgp.SolverState.load(str(tmp_path / "m.npz"))


def test_state_entry_points_validate_without_a_device():
    """NULL plans and bad geometry are refused on the host, in the style of
    test_abi.test_ctypes_load_and_version."""
    import _bsgp
    L = _bsgp.lib()
    for f in ("bsgp_state_layout", "bsgp_state_bytes", "bsgp_state_save", "bsgp_solve_resume"):
        assert f in _bsgp.EXPORTED and hasattr(L, f)
    nb = ctypes.c_int64()
    assert L.bsgp_state_bytes(None, 0, 10, ctypes.byref(nb)) == _bsgp.BSGP_ERR_ARG
    assert b"plan" in L.bsgp_last_error()
    buf = np.zeros(64, np.uint8)
    assert L.bsgp_state_save(None, 1, buf.ctypes.data, 64, None) == _bsgp.BSGP_ERR_ARG
    assert b"plan" in L.bsgp_last_error()
    prm = _bsgp.Params()
    outs = _bsgp.Outputs()
    rc = L.bsgp_solve_resume(None, 1, ctypes.byref(prm), buf.ctypes.data, 1, 64, None,
                             ctypes.byref(outs), None)
    assert rc == _bsgp.BSGP_ERR_ARG and b"plan" in L.bsgp_last_error()
    offs = np.zeros(11, np.int64)
    assert L.bsgp_state_layout(0, 8, 0, 0, 4, offs.ctypes.data) == _bsgp.BSGP_ERR_ARG
    assert L.bsgp_state_layout(8, 8, 5, 0, 4, offs.ctypes.data) == _bsgp.BSGP_ERR_ARG
    assert b"storage" in L.bsgp_last_error()
    assert L.bsgp_state_layout(8, 8, 0, 0, 4, None) == _bsgp.BSGP_ERR_ARG
    assert L.bsgp_abi_version() == 3  # entry points were added, nothing changed


def test_resume_api_refuses_on_the_host():
    """sgp_resume's own argument checks (before any device is touched)."""
    import sgp
    st, *_ = _state()
    with pytest.raises(ValueError, match="gamma"):
        sgp.sgp_resume(st, 30, gamma=1e-3)
    with pytest.raises(ValueError, match="return_state"):
        sgp.sgp_batch(np.ones((2, 8, 8)), np.ones((8, 8)) / 64, 1.0, devices=[0],
                      return_state=True)
    with pytest.raises(ValueError, match="return_state"):
        sgp.sgp_betaDiv_batch(np.ones((2, 8, 8)), np.ones((8, 8)) / 64, 1.0, devices=[0],
                              return_state=True)
