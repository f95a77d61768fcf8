"""ctypes binding of libbsgp.so (include/bsgp.h) — the only way the Python
drop-in reaches the GPU.  There is no CPU fallback: if the library or a
device is missing, every entry point raises ``BsgpError``.

PyTorch is imported *before* the library is loaded so that the process holds
exactly one HIP runtime (torch ships its own ``libamdhip64.so``; the library's
``libamdhip64.so.7`` dependency then binds to it).  Torch is used for device
memory and the current stream only; no torch type crosses the C ABI.
"""
import ctypes
import os
import threading

import numpy as np

try:  # one HIP runtime per process: torch's, loaded first
    import torch  # noqa: F401
except ImportError:  # pragma: no cover - torch is part of the image
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BSGP_LIB", os.path.join(_HERE, "libbsgp.so"))

BSGP_CONV_CIRCULAR = 0
BSGP_CONV_LINEAR_FILL = 1
BSGP_VARIANT_KL = 0
BSGP_VARIANT_BETA = 1
BSGP_STORAGE_F64 = 0
BSGP_STORAGE_F32 = 1
ABI_VERSION = 3
BSGP_ERR_ARG = -1
BSGP_ERR_HIP = -2
BSGP_ERR_UNSUPPORTED = -3
BSGP_ERR_PSF = -4
BSGP_DTYPE_F32 = 0
BSGP_DTYPE_F64 = 1
BSGP_DEBLEND_MAX_BOX = 4096  # box pixels of one parent in LDS (include/bsgp.h)
BSGP_DEBLEND_LARGE_MAX_AREA = 262144  # pixels of one parent on the global-memory path
BSGP_DEBLEND_LINEAR, BSGP_DEBLEND_EXPONENTIAL = 0, 1
BSGP_DEBLEND_OVER_CAP, BSGP_DEBLEND_BAD_LABEL = 1, 2
BSGP_LOCALBKG_MAX = 8192  # values of one local-background annulus in LDS (include/bsgp.h)
BSGP_LOCALBKG_FEW, BSGP_LOCALBKG_OVER_CAP = 1, 2
BSGP_MATCH_LDS_MAX = 4096  # cap1 + cap2 of the cross-match's LDS path (include/bsgp.h)
BSGP_MATCH_MAX = 16384  # rows of one catalogue in a cross-match
BSGP_MATCH_AUTO, BSGP_MATCH_LDS, BSGP_MATCH_GLOBAL = 0, 1, 2
BSGP_MATCH_NONFINITE, BSGP_MATCH_OVER_CAP = 1, 2
# star-stamp status bits (include/bsgp.h): the cutout's, the driver's selection's, the choice's
BSGP_STAMP_PARTIAL, BSGP_STAMP_NO_OVERLAP, BSGP_STAMP_BAD_POSITION = 1, 2, 4
BSGP_STAMP_NO_SOURCE, BSGP_STAMP_MULTI_SOURCE, BSGP_STAMP_BAD_FLUX = 8, 16, 32
BSGP_STAMP_NO_CANDIDATE, BSGP_STAMP_RESTORED_NO_SOURCE = 64, 128
BSGP_STAMP_ROW_COLS = 11  # columns of a bsgp_stamp_select result row
BSGP_VALIDATE_MAX = 16384  # values of one source-validation window in LDS (include/bsgp.h)
# the PSF fit (include/bsgp.h): limits, per-star status bits, the frame's
BSGP_PSFFIT_MAX_COEF, BSGP_PSFFIT_MAX_STARS = 108, 4096
BSGP_PSFFIT_PARTIAL, BSGP_PSFFIT_BAD_POSITION, BSGP_PSFFIT_NO_OVERLAP = 1, 2, 4
BSGP_PSFFIT_FEW_PIXELS, BSGP_PSFFIT_BAD_FLUX, BSGP_PSFFIT_BAD_WEIGHT = 8, 16, 32
BSGP_PSFFIT_CLIPPED, BSGP_PSFFIT_EXCLUDED, BSGP_PSFFIT_SINGULAR = 64, 2 | 4 | 8 | 16 | 32, 128
# star finding (include/bsgp.h): limits, per-star status bits, the frame's, the sky estimators
BSGP_STARFIND_MAX_R, BSGP_STARFIND_MAX = 15, 16384
BSGP_STARFIND_BAD_FLUX, BSGP_STARFIND_OFF_CENTRE = 1, 2
BSGP_STARFIND_FEW_SKY, BSGP_STARFIND_SKY_OVER_CAP = 4, 8
BSGP_STARFIND_REJECTED, BSGP_STARFIND_OVER_CAP = 1 | 2 | 4 | 8, 16
BSGP_STARFIND_BKG_MODE, BSGP_STARFIND_BKG_MEDIAN, BSGP_STARFIND_BKG_MEAN = 0, 1, 2
# status bits of the background-matched co-add (include/bsgp.h)
BSGP_COADD_NONFINITE, BSGP_COADD_ISOLATED, BSGP_COADD_NOT_CONVERGED = 1, 2, 4
# bsgp_convolve2d_ex (include/bsgp.h): kernel size per axis, flags, status bits
BSGP_CONV_MAX_KERNEL = 63
BSGP_CONV_F_INTERPOLATE, BSGP_CONV_F_FILL = 0, 1
BSGP_CONV_F_NORMALIZE, BSGP_CONV_F_PRESERVE_NAN = 2, 4
BSGP_CONV_HAD_NAN, BSGP_CONV_NAN_LEFT = 1, 2


class BsgpError(RuntimeError):
    """A failure reported by libbsgp (status code + bsgp_last_error())."""

    def __init__(self, code, msg):
        super().__init__(f"libbsgp error {code}: {msg}")
        self.code = code


class Params(ctypes.Structure):
    _fields_ = [
        ("variant", ctypes.c_int32), ("init_recon", ctypes.c_int32),
        ("proj_type", ctypes.c_int32), ("stop_criterion", ctypes.c_int32),
        ("MAXIT", ctypes.c_int32), ("M_alpha", ctypes.c_int32), ("M", ctypes.c_int32),
        ("max_projs", ctypes.c_int32),
        ("gamma", ctypes.c_double), ("beta", ctypes.c_double), ("alpha", ctypes.c_double),
        ("alpha_min", ctypes.c_double), ("alpha_max", ctypes.c_double), ("tau", ctypes.c_double),
        ("ccd_sat_level", ctypes.c_double), ("betaParam", ctypes.c_double),
        ("lr", ctypes.c_double), ("lr_exp_param", ctypes.c_double),
        ("tol_convergence", ctypes.c_double), ("prescaled_scaling", ctypes.c_double),
        ("prescaled_tol4", ctypes.c_double),
        ("has_sat", ctypes.c_int32), ("scale_data", ctypes.c_int32), ("verbose", ctypes.c_int32),
        ("adapt_beta", ctypes.c_int32), ("schedule_lr", ctypes.c_int32),
        ("bkg_is_map", ctypes.c_int32), ("ls_spec", ctypes.c_int32), ("ls_series", ctypes.c_int32),
        ("streams", ctypes.c_int32), ("team", ctypes.c_int32), ("proj_cache", ctypes.c_int32),
        ("gn_compact", ctypes.c_int32), ("gn_f32", ctypes.c_int32),
        ("beta0_general", ctypes.c_int32), ("flux_f32", ctypes.c_int32),
        ("persistent", ctypes.c_int32),
    ]


_P = ctypes.c_void_p


class Inputs(ctypes.Structure):
    _fields_ = [("gn", _P), ("bkg", _P), ("flux", _P), ("x0", _P), ("beta0", _P), ("obj", _P)]


class Outputs(ctypes.Structure):
    _fields_ = [("x", _P), ("iters", _P), ("discr", _P), ("times", _P), ("crit", _P),
                ("flags", _P), ("beta_final", _P), ("counters", _P), ("err", _P),
                ("x_iter", _P)]


class PsfModel(ctypes.Structure):
    """bsgp_psf_model (include/bsgp.h)."""
    _fields_ = [("hw", ctypes.c_int32), ("ngauss", ctypes.c_int32), ("ldeg", ctypes.c_int32),
                ("sdeg", ctypes.c_int32), ("cos", ctypes.c_double), ("sin", ctypes.c_double),
                ("ax", ctypes.c_double), ("ay", ctypes.c_double), ("sigma_inc", ctypes.c_double),
                ("x_orig", ctypes.c_double), ("y_orig", ctypes.c_double), ("coeffs", _P),
                ("ncoef", ctypes.c_int32)]


BSGP_STATE_MAGIC = 0x53475342
BSGP_STATE_VERSION = 1
BSGP_STATE_HEADER_BYTES = 1024


class StateHeader(ctypes.Structure):
    """bsgp_state_header (include/bsgp.h): the first bytes of a solver-state record."""
    _fields_ = [
        ("magic", ctypes.c_uint32), ("version", ctypes.c_uint32),
        ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("storage", ctypes.c_int32),
        ("conv_mode", ctypes.c_int32), ("hist_cap", ctypes.c_int32), ("T", ctypes.c_int32),
        ("iters_done", ctypes.c_int32), ("stopped", ctypes.c_int32), ("Xones", ctypes.c_int32),
        ("epoch", ctypes.c_int32), ("g32", ctypes.c_int32), ("beta0_given", ctypes.c_int32),
        ("record_bytes", ctypes.c_int64), ("counters", ctypes.c_int64 * 7),
        ("scaling", ctypes.c_double), ("flux", ctypes.c_double), ("bkg_scalar", ctypes.c_double),
        ("x_low", ctypes.c_double), ("x_upp", ctypes.c_double), ("Dcoeff", ctypes.c_double),
        ("tol", ctypes.c_double), ("elapsed", ctypes.c_double), ("fv", ctypes.c_double),
        ("alpha", ctypes.c_double), ("tau", ctypes.c_double), ("lr", ctypes.c_double),
        ("init_lr", ctypes.c_double), ("beta", ctypes.c_double), ("lam_p", ctypes.c_double),
        ("lam_ratio", ctypes.c_double), ("kappa", ctypes.c_double), ("konst", ctypes.c_double),
        ("gfill", ctypes.c_double), ("Valpha", ctypes.c_double * 32),
        ("Fold", ctypes.c_double * 32), ("prm", Params),
    ]


assert ctypes.sizeof(StateHeader) <= BSGP_STATE_HEADER_BYTES
STATE_HEADER_DTYPE = np.dtype(StateHeader)
# sections of a record after the header, in bsgp_state_layout's order (offs[1:])
STATE_SECTIONS = ("discr", "crit", "times", "flags", "x", "g", "x_tf", "pw", "gn", "bkg")

_lib = None
_lib_lock = threading.Lock()

_i32, _i64, _dbl = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
# Every entry point of include/bsgp.h that returns a status (int): its argument
# types, in the header's order.  lib() sets argtypes and restype from this one
# table and EXPORTED is its keys (plus the two below that return something
# else); tests/test_abi.py holds each entry's length against the declaration.
_ENTRY_POINTS = {
    "bsgp_plan_create": [_i32, _i32, _P, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(_P)],
    "bsgp_plan_create_checked": [_i32, _i32, _P, _i32, _i32, _i32, _i32, _i32, _i32,
                                 ctypes.POINTER(_P)],
    "bsgp_plan_destroy": [_P],
    "bsgp_plan_info": [_P, _P, _P, _P, _P],
    "bsgp_solve_device": [_P, _i32, _P, _P, _P, _P],
    "bsgp_solve_host": [_P, _i32, _P, _P, _P],
    "bsgp_solve_profiled": [_P, _i32, _P, _P, _P, _P, _P, _P],
    "bsgp_apply_operator": [_P, _i32, _i32, _P, _P, _P],
    "bsgp_project_df": [_i64, _dbl, _P, _P, _dbl, _i32, _dbl, _dbl, _dbl, _dbl, _i32, _i32, _i32,
                        _P, _P, _P],
    "bsgp_beta_div": [_i64, _P, _P, _dbl, _P, _P],
    "bsgp_beta_div_deriv": [_i64, _P, _P, _dbl, _P, _P],
    "bsgp_beta_div_grad_parts": [_i64, _P, _P, _dbl, _P, _P, _P],
    "bsgp_device_synchronize": [],
    "bsgp_extract_tiles": [_P, _i32, _i32, _P, _i32, _i32, _i32, _P, _P],
    "bsgp_coadd_tiles": [_P, _i32, _i32, _i32, _P, _i32, _i32, _P, _P, _P],
    "bsgp_tile_offsets": [_P, _i32, _i32, _i32, _P, _P, _i32, _P, _P, _P],
    "bsgp_tile_corrections": [_i32, _P, _P, _P, _P, _P, _i32, _P, _i32, _P, _P, _P, _P],
    "bsgp_coadd_tiles_matched": [_P, _i32, _i32, _i32, _P, _P, _i32, _i32, _P, _P, _P],
    "bsgp_fits_to_f64": [_P, _i64, _i32, _dbl, _dbl, _P, _P],
    "bsgp_psf_stamps": [ctypes.POINTER(PsfModel), _P, _i32, _i32, _i32, _P, _P],
    "bsgp_plan_set_psfs": [_P, _P, _i32, _P],
    "bsgp_plan_set_static_geo": [_P, _i32],
    "bsgp_plan_static_geo": [_P, _P],
    "bsgp_state_layout": [_i32, _i32, _i32, _i32, _i32, _P],
    "bsgp_state_bytes": [_P, _i32, _i32, ctypes.POINTER(_i64)],
    "bsgp_state_save": [_P, _i32, _P, _i64, _P],
    "bsgp_solve_resume": [_P, _i32, _P, _P, _i32, _i64, _P, _P, _P],
    "bsgp_background2d": [_P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _dbl, _i32, _dbl,
                          _i32, _P, _P, _P, _P, _P, _P, _P, _P],
    "bsgp_convolve2d": [_P, _i32, _i32, _i32, _i32, _P, _i32, _i32, _P, _P],
    "bsgp_convolve2d_ex": [_P, _i32, _i32, _i32, _i32, _P, _i32, _i32, _i32, _P, _P, _i32, _dbl,
                           _P, _P, _P],
    "bsgp_detect_sources": [_P, _i32, _i32, _i32, _i32, _P, _dbl, _i32, _i32, _P, _P, _P, _P],
    "bsgp_segment_catalog": [_P, _P, _P, _i32, _i32, _i32, _i32, _P, _P, _P, _P, _P],
    "bsgp_deblend_sources": [_P, _P, _i32, _i32, _i32, _i32, _P, _P, _P, _i32, _i32, _dbl, _i32,
                             _i32, _P, _P, _P, _P],
    "bsgp_deblend_sources_large": [_P, _P, _i32, _i32, _i32, _i32, _P, _P, _P, _i32, _i32, _dbl,
                                   _i32, _i32, _i32, _P, _P, _P, _P],
    "bsgp_segment_local_background": [_P, _i32, _P, _i32, _i32, _i32, _i32, _P, _P, _P, _dbl,
                                      _dbl, _i32, _i32, _i32, _P, _P, _P, _P],
    "bsgp_match_catalogs": [_P, _P, _i32, _P, _i32, _i32, _P, _P, _P, _i32, _P, _i32, _i32, _P,
                            _i32, _dbl, _i32, _P, _P, _P, _P, _P, _P],
    "bsgp_radial_profile": [_P, _i32, _i32, _i32, _i32, _P, _i32, _P, _P, _P],
    "bsgp_fit_gauss1d": [_P, _P, _i32, _i32, _P, _P, _P, _P, _P, _P],
    "bsgp_wasserstein1": [_P, _P, _P, _P, _i32, _i32, _P, _P],
    "bsgp_extract_stamps": [_P, _i32, _i32, _i32, _P, _i32, _i32, _i32, _P, _P, _P, _P],
    "bsgp_stamp_select": [_P, _P, _i32, _P, _i32, _P, _i32, _i32, _P, _P, _P, _P, _P, _P],
    "bsgp_validate_sources": [_P, _i32, _P, _P, _i32, _i32, _i32, _i32, _P, _i32, _P, _i32, _i32,
                              _i32, _dbl, _P, _P, _P, _P],
    "bsgp_psf_fit_moments": [_P, _i32, _i32, _i32, _i32, _P, _P, _i32, ctypes.POINTER(PsfModel),
                             _dbl, _P, _P, _i32, _P, _i32, _dbl, _P, _P, _P, _P, _P, _P, _P],
    "bsgp_psf_fit_solve": [_i32, _i32, _P, _P, ctypes.POINTER(PsfModel), _P, _P, _P, _P, _P, _P,
                           _i32, _dbl, _i32, _P, _P, _P, _P, _P, _P],
    "bsgp_star_maps": [_P, _i32, _i32, _i32, _i32, _P, _P, _P, _i32, _dbl, _P, _P, _P],
    "bsgp_star_peaks": [_P, _i32, _i32, _i32, _i32, _P, _P, _P, _P, _i32, _dbl, _P, _i32, _dbl,
                        _dbl, _i32, _i32, _P, _P, _P, _P],
    "bsgp_star_measure": [_P, _i32, _i32, _i32, _i32, _P, _P, _P, _P, _i32, _P, _P, _i32, _dbl,
                          _dbl, _i32, _dbl, _i32, _i32, _i32, _dbl, _dbl, _P, _P, _P],
    "bsgp_star_select": [_P, _P, _P, _i32, _i32, _i32, _i32, _i32, _dbl, _i32, _dbl, _dbl, _dbl,
                         _i32, _P, _P, _P, _P],
}
EXPORTED = list(_ENTRY_POINTS) + ["bsgp_last_error", "bsgp_abi_version"]


def lib():
    """Load libbsgp.so once; raise loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise BsgpError(-3, f"{LIB_PATH} not built — run __graft_entry__.build()")
            L = ctypes.CDLL(LIB_PATH)
            L.bsgp_last_error.argtypes, L.bsgp_last_error.restype = [], ctypes.c_char_p
            L.bsgp_abi_version.argtypes, L.bsgp_abi_version.restype = [], _i32
            for name, argtypes in _ENTRY_POINTS.items():
                fn = getattr(L, name)
                fn.argtypes, fn.restype = argtypes, ctypes.c_int
            if L.bsgp_abi_version() != ABI_VERSION:
                raise BsgpError(-3, f"{LIB_PATH} has ABI {L.bsgp_abi_version()}, this binding "
                                    f"needs {ABI_VERSION}: rebuild with __graft_entry__.build()")
            _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise BsgpError(rc, lib().bsgp_last_error().decode(errors="replace"))


def require_gpu():
    """The product path runs on the device or not at all."""
    if torch is None or not torch.cuda.is_available():
        raise BsgpError(-2, "no HIP device visible: the beta-SGP engine has no CPU fallback")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def current_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Plan:
    """A device plan: FFT geometry + PSF transfer functions (bsgp_plan_create)."""

    _leased = False  # held by a solve (lease_plan)
    _done = None  # event after the last leased solve's launches

    def __init__(self, H, W, psf, conv_mode, device=None, storage=BSGP_STORAGE_F64,
                 psf_checked=False):
        require_gpu()
        if device is None:
            device = torch.cuda.current_device()
        psf = np.ascontiguousarray(psf, dtype="<f8")
        self.H, self.W = int(H), int(W)
        self.kh, self.kw = psf.shape
        self.conv_mode = conv_mode
        self.device = device
        self.storage = storage
        h = ctypes.c_void_p()
        # psf_checked: the caller has checked the PSF's normalisation itself,
        # in its own dtype (the drop-in's pool and per-image plans, after
        # sgp._check_psf / check_psf_once), so the library's float64 check is
        # skipped; a direct construction keeps the library's check
        rc = lib().bsgp_plan_create_checked(self.H, self.W, psf.ctypes.data, self.kh, self.kw,
                                            conv_mode, storage, device, int(bool(psf_checked)),
                                            ctypes.byref(h))
        if rc != 0:
            raise BsgpError(rc, lib().bsgp_last_error().decode(errors="replace"))
        self.h = h
        P, Q, wave = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        sb = ctypes.c_int64()
        check(lib().bsgp_plan_info(h, ctypes.byref(P), ctypes.byref(Q), ctypes.byref(sb),
                                   ctypes.byref(wave)))
        self.P, self.Q, self.slot_bytes, self.fft_waves = P.value, Q.value, sb.value, wave.value

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and _lib is not None:
            try:
                _lib.bsgp_plan_destroy(h)
            except Exception:  # pragma: no cover
                pass
            self.h = None

    # -------------------------------------------------------------- operators
    def set_psfs(self, psfs):
        """Give image i of every later solve its own PSF psfs[i] ([n, kh, kw]
        float64 CUDA tensor; bsgp_plan_set_psfs builds the n TF pairs on the device)."""
        psfs = psfs.to(dtype=torch.float64).contiguous()
        if psfs.dim() != 3 or tuple(psfs.shape[1:]) != (self.kh, self.kw):
            raise ValueError(f"psfs must be [n, {self.kh}, {self.kw}]")
        check(lib().bsgp_plan_set_psfs(self.h, _ptr(psfs), psfs.shape[0], current_stream()))
        self.n_psf = psfs.shape[0]
        return self

    def set_static_geo(self, mode):
        """The compile-time-geometry path of the persistent solver for the NEXT
        solve / resume on this plan only: None = the default (BSGP_STATIC_GEO,
        else on), 0 / 1 (bsgp_plan_set_static_geo)."""
        check(lib().bsgp_plan_set_static_geo(self.h, -1 if mode is None else int(bool(mode))))
        return self

    def static_geo_used(self):
        """Whether the plan's last solve took that path (bsgp_plan_static_geo)."""
        used = ctypes.c_int32()
        check(lib().bsgp_plan_static_geo(self.h, ctypes.byref(used)))
        return bool(used.value)

    def apply(self, x, transpose=False):
        """A(x) / AT(x) on a [B,H,W] (or [H,W]) float64 CUDA tensor."""
        x = x.contiguous()
        out = torch.empty_like(x)
        B = 1 if x.dim() == 2 else x.shape[0]
        check(lib().bsgp_apply_operator(self.h, B, int(transpose), _ptr(x), _ptr(out),
                                        current_stream()))
        return out

    # ------------------------------------------------------------------ solve
    def solve(self, gn, bkg, params, flux=None, x0=None, beta0=None, want_times=True, obj=None,
              want_iterates=False, profile=False):
        """Batched solve on device tensors: gn [B,H,W] f64; bkg [B] or [B,H,W];
        flux/beta0 [B] or None; x0 [B,H,W] or None; obj [B,H,W] or None (then
        "err" holds the per-iteration relative error); want_iterates adds
        "x_iter" [B,MAXIT,H,W].  Asynchronous on the current stream; returns a
        dict of device output tensors.  profile=True runs bsgp_solve_profiled
        (one stream, synchronous) and adds "kernel_ms" / "launches" [6]: setup,
        k_dir, k_col, k_ls, k_bb, k_persist."""
        B = gn.shape[0]
        M1 = params.MAXIT + 1
        dev = gn.device
        f64 = dict(dtype=torch.float64, device=dev)
        if want_iterates:
            # save=True keeps every iterate of the MAXIT budget on the device
            # (copied to the host once, up to the iterations run): refuse a
            # budget that the device cannot hold beside the solve's own workspace
            need = B * params.MAXIT * self.H * self.W * 8
            free = torch.cuda.mem_get_info(dev)[0]
            if need > 0.8 * free:
                raise BsgpError(
                    f"save=True keeps {params.MAXIT} iterates of {self.H}x{self.W} on the device "
                    f"({need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB free): lower MAXIT")
        # the small outputs are views of two zeroed blocks (two fill launches
        # instead of eight on the latency-bound single-image calls)
        nd = B * M1 * (2 + bool(want_times) + (obj is not None)) + B
        d64 = torch.zeros(nd, **f64)
        i32 = torch.zeros(B * (M1 + 1) + 2 * 8 * B, dtype=torch.int32, device=dev)
        parts = iter(torch.split(d64, [B * M1] * (2 + bool(want_times) + (obj is not None)) + [B]))
        discr, crit = next(parts).view(B, M1), next(parts).view(B, M1)
        times = next(parts).view(B, M1) if want_times else None
        err = next(parts).view(B, M1) if obj is not None else None
        beta_final = next(parts)
        cnt, iters, flags = torch.split(i32, [2 * 8 * B, B, B * M1])  # (int64 counters first: aligned)
        out = {
            "x": torch.empty_like(gn),
            "iters": iters,
            "discr": discr,
            "times": times,
            "crit": crit,
            "flags": flags.view(B, M1),
            "beta_final": beta_final,
            "counters": cnt.view(torch.int64).view(B, 8),
            "err": err,
            "x_iter": (torch.zeros(B, params.MAXIT, self.H, self.W, **f64) if want_iterates
                       else None),
        }
        ins = Inputs(_ptr(gn), _ptr(bkg), _ptr(flux), _ptr(x0), _ptr(beta0), _ptr(obj))
        outs = Outputs(*[_ptr(out[k]) for k in ["x", "iters", "discr", "times", "crit", "flags",
                                                 "beta_final", "counters", "err", "x_iter"]])
        self._keep = (gn, bkg, flux, x0, beta0, obj)
        self._last = (B, int(params.MAXIT), int(params.bkg_is_map), out)
        if profile:
            kms = np.zeros(6, np.float64)
            nl = np.zeros(6, np.int64)
            check(lib().bsgp_solve_profiled(self.h, B, ctypes.byref(params), ctypes.byref(ins),
                                            ctypes.byref(outs), current_stream(),
                                            kms.ctypes.data, nl.ctypes.data))
            out["kernel_ms"], out["launches"] = kms, nl
            return out
        check(lib().bsgp_solve_device(self.h, B, ctypes.byref(params), ctypes.byref(ins),
                                      ctypes.byref(outs), current_stream()))
        return out

    # ------------------------------------------------------- save and resume
    def save_state(self, B):
        """The solver state the last solve / resume of B images left on this
        plan, as a [B, bytes] uint8 CUDA tensor of records (bsgp_state_save).
        Call it before anything else solves on the plan.  Asynchronous."""
        last = getattr(self, "_last", None)
        if last is None or last[0] != B:
            raise BsgpError(BSGP_ERR_ARG, "save_state: no solve of this batch size ran on the plan")
        _, maxit, bmap, _ = last
        nb = ctypes.c_int64()
        check(lib().bsgp_state_bytes(self.h, bmap, maxit, ctypes.byref(nb)))
        rec = torch.empty((B, nb.value), dtype=torch.uint8, device="cuda")
        check(lib().bsgp_state_save(self.h, B, _ptr(rec), nb.value, current_stream()))
        return rec

    def resume(self, state, params, index=None, want_times=True):
        """Continue records (a [n, bytes] uint8 CUDA tensor) up to params.MAXIT
        (bsgp_solve_resume): image i of the result is record index[i] (an int32
        CUDA tensor) or record i.  Returns the dict of :meth:`solve`."""
        n = state.shape[0]
        B = n if index is None else int(index.numel())
        M1 = params.MAXIT + 1
        dev = state.device
        f64 = dict(dtype=torch.float64, device=dev)
        d64 = torch.zeros(B * M1 * (2 + bool(want_times)) + B, **f64)
        i32 = torch.zeros(B * (M1 + 1) + 2 * 8 * B, dtype=torch.int32, device=dev)
        parts = iter(torch.split(d64, [B * M1] * (2 + bool(want_times)) + [B]))
        discr, crit = next(parts).view(B, M1), next(parts).view(B, M1)
        times = next(parts).view(B, M1) if want_times else None
        beta_final = next(parts)
        cnt, iters, flags = torch.split(i32, [2 * 8 * B, B, B * M1])
        out = {
            "x": torch.empty((B, self.H, self.W), **f64),
            "iters": iters, "discr": discr, "times": times, "crit": crit,
            "flags": flags.view(B, M1), "beta_final": beta_final,
            "counters": cnt.view(torch.int64).view(B, 8), "err": None, "x_iter": None,
        }
        outs = Outputs(*[_ptr(out[k]) for k in ["x", "iters", "discr", "times", "crit", "flags",
                                                 "beta_final", "counters", "err", "x_iter"]])
        self._keep = (state, index)
        check(lib().bsgp_solve_resume(self.h, B, ctypes.byref(params), _ptr(state), n,
                                      state.shape[1], _ptr(index), ctypes.byref(outs),
                                      current_stream()))
        self._last = (B, int(params.MAXIT), int(params.bkg_is_map), out)
        return out


def state_layout(H, W, storage, bkg_is_map, hist_cap):
    """Byte offsets of a solver-state record (bsgp_state_layout; needs no
    device): {'bytes': record bytes, 'discr': ..., ..., 'bkg': 0 without a map}."""
    offs = np.zeros(11, np.int64)
    check(lib().bsgp_state_layout(int(H), int(W), int(storage), int(bool(bkg_is_map)),
                                  int(hist_cap), offs.ctypes.data))
    return dict(zip(("bytes",) + STATE_SECTIONS, (int(v) for v in offs)))


class SolverState:
    """The state of a batched solve after its last iteration: one fixed-size
    record per image (include/bsgp.h, bsgp_state_header + sections) plus the
    PSF that finds the plan again.  ``records`` is a [B, bytes] uint8 array, on
    the host (numpy) or on the device (CUDA tensor).  A resume needs nothing
    else: not the observed images, not the original keyword arguments."""

    def __init__(self, records, psf):
        self.records = records
        self.psf = np.ascontiguousarray(psf)
        self._hdr = None

    # ------------------------------------------------------------- accessors
    @property
    def on_device(self):
        return torch is not None and torch.is_tensor(self.records)

    @property
    def header(self):
        """The record headers as a numpy structured array (STATE_HEADER_DTYPE)."""
        if self._hdr is None:
            n = STATE_HEADER_DTYPE.itemsize
            h = self.records[:, :n]
            h = h.cpu().numpy() if self.on_device else np.ascontiguousarray(h)
            self._hdr = h.reshape(-1).view(STATE_HEADER_DTYPE).copy()
        return self._hdr

    def __len__(self):
        return int(self.records.shape[0])

    @property
    def iters_done(self):
        return self.header["iters_done"].copy()

    @property
    def stopped(self):
        """True where the solve has ended (a stop rule or the setup stopped the
        image): a resume leaves those images as they are."""
        return self.header["stopped"] != 0

    @property
    def shape(self):
        h = self.header[0]
        return int(h["H"]), int(h["W"])

    @property
    def layout(self):
        h = self.header[0]
        return state_layout(h["H"], h["W"], h["storage"], h["prm"]["bkg_is_map"], h["hist_cap"])

    def params(self):
        """The ``Params`` of the solve the records come from."""
        return Params.from_buffer_copy(self.header[0]["prm"].tobytes())

    def field(self, name):
        """Section ``name`` of every record as a host array: discr / crit /
        times [B, hist_cap] float64, flags int32, x / g / x_tf / pw [B, H, W]
        in the storage type, gn / bkg [B, H, W] float64 (gn: the slot's bytes,
        see ``header['g32']``)."""
        H, W = self.shape
        L, h = self.layout, self.header[0]
        rec = self.to_host().records
        if name in ("discr", "crit", "times", "flags"):
            dt, n, shp = (np.int32 if name == "flags" else np.float64), int(h["hist_cap"]), None
        else:
            vec = name in ("x", "g", "x_tf", "pw")
            dt = np.float32 if (vec and h["storage"] == BSGP_STORAGE_F32) else np.float64
            n, shp = H * W, (len(self), H, W)
        if name == "bkg" and not L["bkg"]:
            return None
        nb = n * np.dtype(dt).itemsize
        a = np.ascontiguousarray(rec[:, L[name]:L[name] + nb]).view(dt)
        return a.reshape(shp) if shp else a

    def __getitem__(self, idx):
        """Subset / permutation of the images (an index array, a slice or an int)."""
        if isinstance(idx, (int, np.integer)):
            idx = [int(idx)]
        if isinstance(idx, slice):
            idx = np.arange(len(self))[idx]
        idx = np.asarray(idx)
        if idx.dtype == bool:
            idx = np.nonzero(idx)[0]
        idx = idx.astype(np.int64)
        rec = (self.records[torch.as_tensor(idx, device=self.records.device)] if self.on_device
               else self.records[idx])
        return SolverState(rec, self.psf)

    # ------------------------------------------------------- host and device
    def to_host(self):
        if not self.on_device:
            return self
        s = SolverState(self.records.cpu().numpy(), self.psf)
        return s

    def to_device(self):
        if self.on_device:
            return self
        require_gpu()
        return SolverState(torch.from_numpy(np.ascontiguousarray(self.records)).to("cuda"),
                           self.psf)

    # ------------------------------------------------------------------ disk
    def save(self, path):
        """One .npz: the records, the PSF and the layout version."""
        h = self.to_host()
        with open(path, "wb") as f:
            np.savez(f, records=h.records, psf=h.psf,
                     version=np.int64(BSGP_STATE_VERSION),
                     shape=np.asarray(h.shape, np.int64))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            if int(z["version"]) != BSGP_STATE_VERSION:
                raise ValueError(f"{path}: solver-state layout version {int(z['version'])}, "
                                 f"this library reads version {BSGP_STATE_VERSION}")
            rec, psf, shape = z["records"], z["psf"], tuple(int(v) for v in z["shape"])
        s = cls(rec, psf)
        s.validate(shape)
        return s

    def validate(self, shape=None):
        """Raise ValueError unless every record carries the magic number, this
        library's layout version, one shape (``shape`` if given) and the size
        its own header implies."""
        rec = self.records
        if rec.ndim != 2 or rec.shape[0] < 1 or rec.shape[1] < BSGP_STATE_HEADER_BYTES:
            raise ValueError("solver state: records must be [B, bytes] uint8")
        h = self.header
        if np.any(h["magic"] != BSGP_STATE_MAGIC):
            raise ValueError("solver state: bad magic number (not a solver-state record)")
        if np.any(h["version"] != BSGP_STATE_VERSION):
            raise ValueError(f"solver state: layout version {int(h['version'][0])}, this library "
                             f"reads version {BSGP_STATE_VERSION}")
        H, W = self.shape
        if np.any(h["H"] != H) or np.any(h["W"] != W) or (shape is not None
                                                         and tuple(shape) != (H, W)):
            raise ValueError(f"solver state: shape mismatch (records {H}x{W}, expected {shape})")
        if np.any(h["record_bytes"] != rec.shape[1]) or self.layout["bytes"] != rec.shape[1]:
            raise ValueError("solver state: record size does not match its header (shape, "
                             "storage, hist_cap)")

    # ----------------------------------------------------------- construction
    @classmethod
    def from_arrays(cls, psf, params, x, g, x_tf, gn, *, iters_done, alpha, tau, fv, flux,
                    scaling, x_low, x_upp, tol, Valpha, Fold, pw=None, bkg=0.0, beta=None,
                    lr=None, init_lr=None, epoch=None, konst=0.0, Xones=False, stopped=0,
                    lam_p=0.0, lam_ratio=0.0, kappa=0.0, elapsed=0.0, counters=None, discr=None,
                    crit=None, times=None, flags=None, hist_cap=None, team=1,
                    conv_mode=BSGP_CONV_CIRCULAR, storage="f64", beta0_given=False):
        """Records from explicit arrays and scalars (the teacher-forced tests:
        a state captured in the reference, continued on the device).

        Vectors are [B, H, W] (or [H, W] for one image) in *scaled* units, as
        the loop carries them: ``x`` the iterate, ``g`` its gradient, ``x_tf``
        = A(x), ``gn`` the scaled observed image with its null pixels filled,
        ``pw`` = (x_tf + bkg)**(beta - 1) for the beta objective, ``bkg`` a
        scalar per image or a [B, H, W] map.  Scalars are per image ([B] or
        broadcast): ``iters_done`` completed iterations, the step length
        ``alpha``, ``tau``, the objective ``fv`` at x, ``flux``, ``scaling``,
        the scaling-matrix bounds ``x_low`` / ``x_upp``, the stop tolerance
        ``tol``, the memories ``Valpha`` [B, M_alpha] and ``Fold`` [B, M],
        ``beta`` / ``lr`` / ``init_lr`` / ``epoch`` (default: params.betaParam,
        params.lr, params.lr, iters_done), ``konst`` the lambda-independent
        objective sum at beta (sum s*gn**beta over sum gn; 0 for KL), ``Xones``
        (the scaling matrix is still ones).  ``params`` is the ``Params`` of the
        solve; history rows (discr, crit, times, flags: [B, iters_done + 1])
        default to zeros."""
        x = np.asarray(x, np.float64)
        if x.ndim == 2:
            x = x[None]
        Bn, H, W = x.shape
        N = H * W
        sc = storage_code(storage)
        vdt = np.float32 if sc == BSGP_STORAGE_F32 else np.float64
        done = np.broadcast_to(np.asarray(iters_done, np.int64), (Bn,))
        cap = int(hist_cap) if hist_cap is not None else int(done.max()) + 1
        bkg = np.asarray(bkg, np.float64)
        bmap = bkg.ndim >= 2
        prm = Params.from_buffer_copy(bytes(params))
        prm.bkg_is_map = int(bmap)
        L = state_layout(H, W, sc, bmap, cap)
        rec = np.zeros((Bn, L["bytes"]), np.uint8)
        hdr = np.zeros(Bn, STATE_HEADER_DTYPE)

        def per(v, dt=np.float64):
            return np.broadcast_to(np.asarray(v, dt), (Bn,))

        hdr["magic"], hdr["version"] = BSGP_STATE_MAGIC, BSGP_STATE_VERSION
        hdr["H"], hdr["W"], hdr["storage"], hdr["conv_mode"] = H, W, sc, conv_mode
        hdr["hist_cap"], hdr["T"], hdr["iters_done"] = cap, team, done
        hdr["stopped"], hdr["Xones"] = per(stopped, np.int32), per(Xones, np.int32)
        hdr["epoch"] = done if epoch is None else per(epoch, np.int32)
        hdr["beta0_given"] = int(bool(beta0_given))
        hdr["record_bytes"] = L["bytes"]
        if counters is not None:
            hdr["counters"] = np.broadcast_to(np.asarray(counters, np.int64), (Bn, 7))
        hdr["scaling"], hdr["flux"] = per(scaling), per(flux)
        hdr["bkg_scalar"] = 0.0 if bmap else per(bkg)
        hdr["x_low"], hdr["x_upp"], hdr["tol"] = per(x_low), per(x_upp), per(tol)
        hdr["Dcoeff"] = 2 / float(N) * per(scaling)
        hdr["elapsed"], hdr["fv"], hdr["alpha"], hdr["tau"] = per(elapsed), per(fv), per(alpha), per(tau)
        hdr["lr"] = per(prm.lr if lr is None else lr)
        hdr["init_lr"] = per(prm.lr if init_lr is None else init_lr)
        hdr["beta"] = per(prm.betaParam if beta is None else beta)
        hdr["lam_p"], hdr["lam_ratio"], hdr["kappa"] = per(lam_p), per(lam_ratio), per(kappa)
        hdr["konst"] = per(konst)
        va = np.broadcast_to(np.asarray(Valpha, np.float64), (Bn, prm.M_alpha))
        fo = np.broadcast_to(np.asarray(Fold, np.float64), (Bn, prm.M))
        hdr["Valpha"][:, :prm.M_alpha] = va
        hdr["Fold"][:, :prm.M] = fo
        hdr["prm"] = np.frombuffer(bytes(prm), STATE_HEADER_DTYPE["prm"])[0]
        rec[:, :STATE_HEADER_DTYPE.itemsize] = hdr.view(np.uint8).reshape(Bn, -1)

        def put(name, a, dt):
            if a is None:
                return
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dt), (Bn, H, W))
                                     if name in ("x", "g", "x_tf", "pw", "gn", "bkg")
                                     else np.asarray(a, dt).reshape(Bn, -1))
            b = a.reshape(Bn, -1).view(np.uint8)
            rec[:, L[name]:L[name] + b.shape[1]] = b

        put("x", x, vdt)
        put("g", g, vdt)
        put("x_tf", x_tf, vdt)
        put("pw", pw, vdt)
        put("gn", gn, np.float64)
        if bmap:
            put("bkg", bkg, np.float64)
        for name, a in (("discr", discr), ("crit", crit), ("times", times)):
            if a is not None:
                put(name, np.asarray(a, np.float64)[..., :cap], np.float64)
        if flags is not None:
            put("flags", np.asarray(flags, np.int32)[..., :cap], np.int32)
        s = cls(rec, psf)
        s.validate()
        return s


STATUS_LS_CAP = 1
STATUS_TEAM_TIMEOUT = 4
STATUS_NO_POSITIVE_BOUND = 8


def check_status(counters):
    """Raise if a solve reported a status bit in counters[:, 3]: its results
    are not valid.  Bit 1: the line search hit its trial cap, which happens
    only for a backtracking factor outside (0, 1), where the reference's
    loop (sgp.py:328-349 / 776-801) never terminates; bit 4: a team barrier
    timed out (workgroups not co-resident); bit 8: y = flux/(flux+bkg)*AT(gn)
    has no positive entry, where the reference raises numpy's ValueError
    (np.min of an empty array, sgp.py:269-270 / 711-712) -- raised here as
    ValueError too."""
    c = counters.cpu().numpy() if hasattr(counters, "cpu") else np.asarray(counters)
    st = c[:, 3]
    if np.any(st & STATUS_NO_POSITIVE_BOUND):
        bad = np.nonzero(st & STATUS_NO_POSITIVE_BOUND)[0].tolist()
        raise ValueError("zero-size array to reduction operation minimum which has no identity "
                         f"(image(s) {bad[:8]}: y = flux/(flux+bkg)*AT(gn) has no positive "
                         "entry, sgp.py:269-270)")
    if np.any(st & STATUS_TEAM_TIMEOUT):
        raise BsgpError(BSGP_ERR_HIP, "team barrier timed out (workgroups not co-resident)")
    if np.any(st & STATUS_LS_CAP):
        raise BsgpError(BSGP_ERR_ARG, "line search did not terminate: the backtracking factor "
                                      "beta must lie in (0, 1) (sgp.py:349 lam = lam * beta)")


_plan_cache = {}
_plan_cache_lock = threading.Lock()


STORAGE = {"f64": BSGP_STORAGE_F64, "f32": BSGP_STORAGE_F32}


def storage_code(storage):
    """'f64' / 'f32' (or the BSGP_STORAGE_* value) -> BSGP_STORAGE_*."""
    if storage in STORAGE.values():
        return storage
    if storage not in STORAGE:
        raise ValueError(f"storage must be 'f64' or 'f32', not {storage!r}")
    return STORAGE[storage]


# Plans are found by PSF content.  Keying the cache by the PSF's bytes cost
# every call a copy and a hash of the whole PSF (C4's circular A takes a
# 2048^2 PSF: ~20 ms of host time per call, GPU idle when the call starts
# from an idle stream); the key holds a fingerprint of a strided sample
# instead, and a plan matches only when its own copy of the PSF is
# byte-identical to the caller's (memcmp: one pass over the PSF).
_libc = ctypes.CDLL(None)
_libc.memcmp.restype = ctypes.c_int
_libc.memcmp.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]


def _same_psf(plan, psf):
    ref = plan._psf_host
    return ref.shape == psf.shape and (
        psf.nbytes == 0 or _libc.memcmp(ref.ctypes.data, psf.ctypes.data, psf.nbytes) == 0)


# plan-layout overrides read by bsgp_plan_create (A/B knobs): part of the key,
# so a pooled plan never keeps the layout of an earlier setting
_PLAN_KNOBS = ("BSGP_PERWAVE_MIN_WG", "BSGP_PERWAVE_TW", "BSGP_COOP_ELEMS", "BSGP_LS_PREDICT")


def _plan_key(H, W, psf, conv_mode, storage):
    psf = np.ascontiguousarray(psf, dtype="<f8")
    flat = psf.reshape(-1)
    sample = flat[::max(1, flat.size // 4096)].tobytes()
    return psf, (H, W, psf.shape, hash(sample), conv_mode, storage_code(storage),
                 torch.cuda.current_device(), tuple(os.environ.get(k) for k in _PLAN_KNOBS))


def _new_plan(H, W, psf, key):
    p = Plan(H, W, psf, key[4], key[6], storage=key[5], psf_checked=True)
    p._psf_host = psf.copy()  # (the caller may rewrite its array later)
    return p


def get_plan(H, W, psf, conv_mode, storage="f64"):
    """A plan for the calling thread's own use (operators, plan queries):
    cached per (shape, psf content, mode, storage, device, host thread), since a
    plan's operator workspace serves one call at a time (include/bsgp.h: a
    plan is not thread-safe).  Entries of threads that have ended are dropped.
    Solves take their plan from the shared pool (lease_plan) instead."""
    require_gpu()
    psf, key = _plan_key(H, W, psf, conv_mode, storage)
    key = key + (threading.get_ident(),)
    with _plan_cache_lock:
        p = _plan_cache.get(key)
        if p is None or not _same_psf(p, psf):
            live = {t.ident for t in threading.enumerate()}
            for k in [k for k in _plan_cache if k[-1] not in live]:
                del _plan_cache[k]
            if len(_plan_cache) > 16:
                _plan_cache.clear()
            p = _new_plan(H, W, psf, key)
            _plan_cache[key] = p
    return p


# Solve plans: a pool per (shape, psf, mode, storage, device).  A solve leases
# an idle plan (or creates one) for the duration of its enqueue; the plan's
# workspace stays in use on the device until the solve's stream gets there, so
# the lease ends with an event on that stream and the next lessee's stream
# waits for it.  Concurrent solves (devices=[...] threads, several shards on
# one GPU) get separate plans; later calls reuse them, whichever thread runs
# them, so a new devices=[...] call re-allocates nothing.
_pool = {}
_POOL_MAX = 8  # plans kept per key


_checked = {}  # PSFs that passed a check: (check, dtype, shape, sample hash) -> copy


def check_psf_once(psf, check):
    """Run ``check(psf)`` on the caller's own array (its dtype kept: the
    reference sums the PSF in its own dtype, sgp.py:97-102 / :557-562) unless
    a byte-identical PSF of the same dtype has passed it before.  Found like
    the plans: a fingerprint of a strided sample, then memcmp."""
    psf = np.ascontiguousarray(psf)
    flat = psf.reshape(-1)
    key = (check, psf.dtype.str, psf.shape, hash(flat[::max(1, flat.size // 4096)].tobytes()))
    with _plan_cache_lock:
        ref = _checked.get(key)
        if ref is not None and (psf.nbytes == 0 or _libc.memcmp(
                ref.ctypes.data, psf.ctypes.data, psf.nbytes) == 0):
            return
    check(psf)
    with _plan_cache_lock:
        if len(_checked) > 32:
            _checked.clear()
        _checked[key] = psf.copy()


class lease_plan:
    """Context manager: ``with lease_plan(H, W, psf, mode, storage) as plan``."""

    def __init__(self, H, W, psf, conv_mode, storage="f64"):
        require_gpu()
        self.args = (H, W, psf, conv_mode, storage)
        self.plan = None

    def __enter__(self):
        H, W, psf, conv_mode, storage = self.args
        psf, key = _plan_key(H, W, psf, conv_mode, storage)
        with _plan_cache_lock:
            plans = _pool.setdefault(key, [])
            p = next((q for q in plans if not q._leased and _same_psf(q, psf)), None)
            if p is None:
                p = _new_plan(H, W, psf, key)
                p._done = None
                if len(plans) < _POOL_MAX:
                    plans.append(p)
            p._leased = True
        if p._done is not None:
            torch.cuda.current_stream().wait_event(p._done)
        self.plan = p
        return p

    def __exit__(self, *exc):
        p = self.plan
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        p._done = ev
        with _plan_cache_lock:
            p._leased = False
        return False


def per_image_plan(H, W, psfs, conv_mode, storage="f64"):
    """A plan whose image i uses psfs[i] ([B, kh, kw], numpy or CUDA tensor);
    not cached (it holds B transfer-function pairs)."""
    require_gpu()
    # on the current device whatever device (or host) the stamps come from:
    # the plan-building kernels read them there
    dev = (psfs.to(device=torch.cuda.current_device(), dtype=torch.float64).contiguous()
           if torch.is_tensor(psfs) else to_dev(psfs))
    p = Plan(H, W, dev[0].cpu().numpy(), conv_mode, storage=storage_code(storage),
             psf_checked=True)
    return p.set_psfs(dev)


def to_dev(a):
    a = np.ascontiguousarray(a, dtype="<f8")
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a).to("cuda")


def to_dev_async(a):
    """Host array -> float64 device tensor through page-locked memory (torch's
    caching host allocator, which does not hand the block out again before
    the copy has run), enqueued on the current stream without waiting: the
    single-image drop-in's inputs (a pageable copy stages through the
    runtime's own buffer and blocks)."""
    a = np.asarray(a, dtype="<f8")
    h = torch.empty(a.shape, dtype=torch.float64, pin_memory=True)
    h.numpy()[...] = a
    return h.to("cuda", non_blocking=True)


def to_host(tensors):
    """Device tensors (dict; None entries kept) -> numpy arrays: every copy
    enqueued on the current stream into page-locked memory, ONE stream
    synchronisation, then plain numpy copies (nothing page-locked escapes to
    the caller)."""
    pinned = {k: (None if t is None else t.to("cpu", non_blocking=True))
              for k, t in tensors.items()}
    torch.cuda.current_stream().synchronize()
    return {k: (None if t is None else t.numpy().copy()) for k, t in pinned.items()}


def project_df_dev(b, c, dia, scaling, ccd_sat_level, lambda_, dlambda_, tol_lam, biter, siter,
                   max_projs):
    """flux_conserve_proj.projectDF on device tensors; returns (x, info[4])."""
    x = torch.empty_like(c)
    info = torch.zeros(4, dtype=torch.float64, device=c.device)
    has_sat = ccd_sat_level is not None
    check(lib().bsgp_project_df(c.numel(), float(b), _ptr(c), _ptr(dia), float(scaling),
                                int(has_sat), float(ccd_sat_level) if has_sat else 0.0,
                                float(lambda_), float(dlambda_), float(tol_lam), int(biter),
                                int(siter), int(max_projs), _ptr(x), _ptr(info),
                                current_stream()))
    return x, info


def beta_div_dev(y, x, beta):
    out = torch.zeros(1, dtype=torch.float64, device=y.device)
    check(lib().bsgp_beta_div(y.numel(), _ptr(y), _ptr(x), float(beta), _ptr(out),
                              current_stream()))
    return out


def beta_div_deriv_dev(y, x, beta):
    out = torch.empty_like(y)
    check(lib().bsgp_beta_div_deriv(y.numel(), _ptr(y), _ptr(x), float(beta), _ptr(out),
                                    current_stream()))
    return out


def grad_parts_dev(den, gn, beta):
    p1 = torch.empty_like(den)
    w = torch.empty_like(den)
    check(lib().bsgp_beta_div_grad_parts(den.numel(), _ptr(den), _ptr(gn), float(beta), _ptr(p1),
                                         _ptr(w), current_stream()))
    return p1, w
