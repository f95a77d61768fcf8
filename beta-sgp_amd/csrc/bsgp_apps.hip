// bsgp_apps.hip — the entry points of the C-ABI host layer that take no plan
// (declared in include/bsgp.h): the projection, tiles and their background-matched
// co-add, FITS pixels, PSF stamps,
// sky background, convolution, detection, catalogue, local background,
// deblending, catalogue cross-match, star-stamp metrics, cutouts and selection,
// source validation, the PSF fit, star finding, and the divergences.
// Each validates its arguments and launches its kernels.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "bsgp_host.hpp"
#include "bsgp_psf.hpp"

using namespace bsgp;

namespace {
// the element type of an image argument: float32 or float64
int check_dtype(int32_t dtype) {
  if (dtype != BSGP_DTYPE_F32 && dtype != BSGP_DTYPE_F64)
    return fail(BSGP_ERR_ARG, "dtype must be BSGP_DTYPE_F32 or BSGP_DTYPE_F64");
  return BSGP_OK;
}
}  // namespace

extern "C" {

int bsgp_project_df(int64_t n, double b, const double* c, const double* dia, double scaling,
                    int32_t has_sat, double ccd_sat_level, double lambda0, double dlambda0,
                    double tol_lam, int32_t biter, int32_t siter, int32_t max_projs, double* x,
                    double* info, void* stream) {
  if (n < 1 || n > 0x7fffffff || !c || !dia || !x || !info)
    return fail(BSGP_ERR_ARG, "bad arguments");
  ProjClip clip{has_sat != 0, ccd_sat_level / scaling - 2.220446049250313e-16};
  HIP_TRY(launch_project_df((int)n, b, c, dia, clip, lambda0, dlambda0, tol_lam, biter, siter,
                            max_projs, x, info, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_extract_tiles(const double* img, int32_t H, int32_t W, const int32_t* boxes, int32_t n,
                       int32_t th, int32_t tw, double* out, void* stream) {
  if (!img || !boxes || !out || H < 1 || W < 1 || n < 1 || th < 1 || tw < 1 || th > H || tw > W)
    return fail(BSGP_ERR_ARG, "bad arguments");
  if ((int64_t)n * th > 0x7fffffff) return fail(BSGP_ERR_ARG, "too many tile rows");
  HIP_TRY(launch_extract_tiles(img, W, boxes, n, th, tw, out, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_coadd_tiles(const double* tiles, int32_t n, int32_t th, int32_t tw, const int32_t* boxes,
                     int32_t H, int32_t W, double* mean, double* footprint, void* stream) {
  if (!tiles || !boxes || !mean || H < 1 || W < 1 || n < 1 || n > 8192 || th < 1 || tw < 1)
    return fail(BSGP_ERR_ARG, "bad arguments");
  HIP_TRY(launch_coadd_tiles(tiles, n, th, tw, boxes, H, W, mean, footprint, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_tile_offsets(const double* tiles, int32_t n, int32_t th, int32_t tw, const int32_t* boxes,
                      const int32_t* pairs, int32_t npairs, double* offsets, int32_t* status,
                      void* stream) {
  if (n < 1 || n > 8192 || th < 1 || tw < 1 || npairs < 0)
    return fail(BSGP_ERR_ARG, "bad arguments");
  if ((int64_t)th * tw > 0x7fffffffLL)
    return fail(BSGP_ERR_UNSUPPORTED, "a tile holds fewer than 2^31 pixels (th * tw < 2^31)");
  if (!tiles || !boxes || !status) return fail(BSGP_ERR_ARG, "tiles / boxes / status is NULL");
  if (npairs > 0 && (!pairs || !offsets)) return fail(BSGP_ERR_ARG, "pairs / offsets is NULL");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(status, 0, (size_t)n * sizeof(int), s));
  if (npairs == 0) return BSGP_OK;
  CoaddOffsetArgs a{};
  a.tiles = tiles, a.boxes = boxes, a.pairs = pairs;
  a.n = n, a.th = th, a.tw = tw, a.npairs = npairs;
  a.offsets = offsets, a.status = status;
  HIP_TRY(launch_pair_offsets(a, s));
  return BSGP_OK;
}

int bsgp_tile_corrections(int32_t n, const int32_t* row_ptr, const int32_t* nbr,
                          const int32_t* nbr_pair, const int32_t* nbr_sign,
                          const int32_t* component, int32_t ncomp, const double* offsets,
                          int32_t background_reference, double* corrections, int32_t* status,
                          double* solve_info, void* stream) {
  if (n < 1 || n > 8192 || ncomp < 1 || ncomp > n) return fail(BSGP_ERR_ARG, "bad arguments");
  if (background_reference >= n)
    return fail(BSGP_ERR_ARG, "background_reference must be a tile index (or < 0 for none)");
  // (nbr, nbr_pair, nbr_sign and offsets are empty, and may be NULL, when no tile has a pair)
  if (!row_ptr || !component || !corrections || !status)
    return fail(BSGP_ERR_ARG, "row_ptr / component / corrections / status is NULL");
  CoaddSolveArgs a{};
  a.n = n, a.ncomp = ncomp, a.bref = background_reference < 0 ? -1 : background_reference;
  a.row_ptr = row_ptr, a.nbr = nbr, a.nbr_pair = nbr_pair, a.nbr_sign = nbr_sign;
  a.component = component, a.offsets = offsets;
  a.c = corrections, a.status = status, a.info = solve_info;
  hipStream_t s = (hipStream_t)stream;
  // stream-ordered workspace: the call stays asynchronous
  StreamScratch w(s);
  if (int rc = w.alloc(2 * (size_t)n * sizeof(double))) return rc;
  a.ws = static_cast<double*>(w.p);
  return w.finish(launch_solve_corrections(a, s), "corrections");
}

int bsgp_coadd_tiles_matched(const double* tiles, int32_t n, int32_t th, int32_t tw,
                             const int32_t* boxes, const double* corrections, int32_t H, int32_t W,
                             double* mean, double* footprint, void* stream) {
  if (!tiles || !boxes || !corrections || !mean || H < 1 || W < 1 || n < 1 || n > 8192 ||
      th < 1 || tw < 1)
    return fail(BSGP_ERR_ARG, "bad arguments");
  HIP_TRY(launch_coadd_tiles_matched(tiles, n, th, tw, boxes, corrections, H, W, mean, footprint,
                                     (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_fits_to_f64(const void* raw, int64_t n, int32_t bitpix, double bscale, double bzero,
                     double* out, void* stream) {
  if (!raw || !out || n < 0) return fail(BSGP_ERR_ARG, "bad arguments");
  if (bitpix != 8 && bitpix != 16 && bitpix != 32 && bitpix != 64 && bitpix != -32 &&
      bitpix != -64)
    return fail(BSGP_ERR_ARG, "BITPIX must be 8, 16, 32, 64, -32 or -64");
  if (n == 0) return BSGP_OK;
  HIP_TRY(launch_fits_to_f64(raw, n, bitpix, bscale, bzero, out, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_psf_stamps(const bsgp_psf_model* m, const double* xy, int32_t n, int32_t spatial,
                    int32_t normalize, double* out, void* stream) {
  if (!m || !out || n < 0 || (spatial && !xy) || !m->coeffs)
    return fail(BSGP_ERR_ARG, "bad arguments");
  if (m->hw < 0 || m->hw > 255 || m->ngauss < 1 || m->ldeg < 0 || m->sdeg < 0)
    return fail(BSGP_ERR_ARG, "bad PSF model degrees or half width");
  PsfModel M{};
  M.ncomp = m->ngauss * (m->ldeg + 1) * (m->ldeg + 2) / 2;
  const int nterm = (m->sdeg + 1) * (m->sdeg + 2) / 2;
  const int need = spatial ? M.ncomp * nterm : M.ncomp;
  if (M.ncomp > kPsfMaxLocal || need > kPsfMaxCoef)
    return fail(BSGP_ERR_ARG, "PSF model has too many coefficients");
  if (m->ncoef < need) return fail(BSGP_ERR_ARG, "too few PSF coefficients for the degrees");
  if (n == 0) return BSGP_OK;
  M.cosv = m->cos;
  M.sinv = m->sin;
  M.ax = m->ax;
  M.ay = m->ay;
  M.sig2 = m->sigma_inc * m->sigma_inc;
  M.x_orig = m->x_orig;
  M.y_orig = m->y_orig;
  M.ngauss = m->ngauss;
  M.ldeg = m->ldeg;
  M.sdeg = m->sdeg;
  M.hw = m->hw;
  M.ncoef = need;
  for (int i = 0; i < need; ++i) M.coef[i] = m->coeffs[i];
  HIP_TRY(launch_psf_stamps(M, xy, n, spatial ? 1 : 0, normalize ? 1 : 0, out,
                            (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_background2d(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t bh,
                      int32_t bw, int32_t fh, int32_t fw, double sigma, int32_t maxiters,
                      double exclude_percentile, int32_t clip, const uint8_t* mask, double* bkg_out,
                      double* rms_out, double* mesh_out, double* rms_mesh_out, double* medians_out,
                      int32_t* status_out, void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (int rc = check_dtype(dtype)) return rc;
  if (B < 1 || H < 1 || W < 1) return fail(BSGP_ERR_ARG, "B, H and W must be >= 1");
  if (bh < 1 || bw < 1) return fail(BSGP_ERR_ARG, "box size (bh, bw) must be >= 1");
  if (fh < 1 || fw < 1 || fh % 2 == 0 || fw % 2 == 0)
    return fail(BSGP_ERR_ARG, "filter size (fh, fw) must be odd and >= 1");
  if (!(sigma >= 0.0)) return fail(BSGP_ERR_ARG, "sigma must be >= 0");
  if (maxiters < 0) return fail(BSGP_ERR_ARG, "maxiters must be >= 0");
  if (!(exclude_percentile >= 0.0 && exclude_percentile <= 100.0))
    return fail(BSGP_ERR_ARG, "exclude_percentile must be in [0, 100]");
  char msg[192];
  if ((int64_t)bh * bw > kBkgMaxBox) {
    snprintf(msg, sizeof msg, "box of %lld pixels: a box holds at most %d (bh * bw <= %d)",
             (long long)bh * bw, kBkgMaxBox, kBkgMaxBox);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (fh > kBkgMaxFilter || fw > kBkgMaxFilter) {
    snprintf(msg, sizeof msg, "filter window larger than %d x %d", kBkgMaxFilter, kBkgMaxFilter);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  const int64_t ny = (H + (int64_t)bh - 1) / bh, nx = (W + (int64_t)bw - 1) / bw;
  if (ny * nx > kBkgMaxCells) {
    snprintf(msg, sizeof msg, "mesh of %lld cells: an image's mesh holds at most %d",
             (long long)(ny * nx), kBkgMaxCells);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (B > 65535 || H > 65535)
    return fail(BSGP_ERR_UNSUPPORTED, "B and H must be at most 65535");
  const size_t ncell = (size_t)(ny * nx);
  BkgArgs a{};
  a.data = data;
  a.mask = mask;
  a.B = B, a.H = H, a.W = W, a.bh = bh, a.bw = bw, a.fh = fh, a.fw = fw;
  a.ny = (int)ny, a.nx = (int)nx, a.maxiters = maxiters, a.clip = clip ? 1 : 0;
  a.sigma = sigma;
  a.excl_count = exclude_percentile / 100.0 * (double)(bh * bw);
  a.ws_stride = 6 * ncell + 8;
  a.bkg = bkg_out, a.rms = rms_out, a.mesh = mesh_out, a.rms_mesh = rms_mesh_out;
  a.medians = medians_out, a.status = status_out;
  hipStream_t s = (hipStream_t)stream;
  // stream-ordered workspace: the call stays asynchronous
  const size_t wsb = (size_t)B * a.ws_stride * sizeof(double);
  const size_t wib = (size_t)B * (1 + 3 * ncell) * sizeof(int);
  StreamScratch w(s);
  if (int rc = w.alloc(wsb + wib)) return rc;
  a.ws = static_cast<double*>(w.p);
  a.wsi = reinterpret_cast<int*>(static_cast<char*>(w.p) + wsb);
  hipError_t e = launch_bkg_boxstats(a, dtype == BSGP_DTYPE_F32, s);
  if (e == hipSuccess) e = launch_bkg_mesh(a, s);
  if (e == hipSuccess && (bkg_out || rms_out)) e = launch_bkg_zoom(a, s);
  return w.finish(e, "background");
}

namespace {
// shape checks shared by the segmentation entry points
int seg_shape(int32_t B, int32_t H, int32_t W) {
  if (B < 1 || H < 1 || W < 1) return fail(BSGP_ERR_ARG, "B, H and W must be >= 1");
  if ((int64_t)H * W > 0x7fffffffLL)
    return fail(BSGP_ERR_UNSUPPORTED, "an image holds fewer than 2^31 pixels (H * W < 2^31)");
  if (B > 65535) return fail(BSGP_ERR_UNSUPPORTED, "B must be at most 65535");
  return BSGP_OK;
}
}  // namespace

int bsgp_convolve2d(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                    const double* kernel, int32_t kh, int32_t kw, double* out, void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!kernel) return fail(BSGP_ERR_ARG, "kernel is NULL");
  if (!out) return fail(BSGP_ERR_ARG, "out is NULL");
  if (int rc = check_dtype(dtype)) return rc;
  if (kh < 1 || kw < 1) return fail(BSGP_ERR_ARG, "kernel size (kh, kw) must be >= 1");
  if (int rc = seg_shape(B, H, W)) return rc;
  if (kh % 2 == 0 || kw % 2 == 0 || kh > kSegMaxKernel || kw > kSegMaxKernel) {
    char msg[128];
    snprintf(msg, sizeof msg, "kernel of %d x %d: kernels are odd and at most %d x %d", kh, kw,
             kSegMaxKernel, kSegMaxKernel);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (H > 65535) return fail(BSGP_ERR_UNSUPPORTED, "H must be at most 65535");
  SegConvArgs a{};
  a.data = data, a.kernel = kernel, a.out = out;
  a.B = B, a.H = H, a.W = W, a.kh = kh, a.kw = kw;
  HIP_TRY(launch_seg_convolve(a, dtype == BSGP_DTYPE_F32, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_convolve2d_ex(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                       const double* kernel, int32_t kh, int32_t kw, int32_t kernel_stride,
                       const double* kernel_sum, const uint8_t* mask, int32_t flags,
                       double fill_value, double* out, int32_t* status_out, void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!kernel) return fail(BSGP_ERR_ARG, "kernel is NULL");
  if (!kernel_sum) return fail(BSGP_ERR_ARG, "kernel_sum is NULL");
  if (!out) return fail(BSGP_ERR_ARG, "out is NULL");
  if (!status_out) return fail(BSGP_ERR_ARG, "status_out is NULL");
  if (int rc = check_dtype(dtype)) return rc;
  if (kh < 1 || kw < 1) return fail(BSGP_ERR_ARG, "kernel size (kh, kw) must be >= 1");
  if (flags & ~(BSGP_CONV_F_FILL | BSGP_CONV_F_NORMALIZE | BSGP_CONV_F_PRESERVE_NAN))
    return fail(BSGP_ERR_ARG, "flags holds an unknown bit");
  if (!std::isfinite(fill_value)) return fail(BSGP_ERR_ARG, "fill_value must be finite");
  if (int rc = seg_shape(B, H, W)) return rc;
  if (kh % 2 == 0 || kw % 2 == 0 || kh > kConvMaxKernel || kw > kConvMaxKernel) {
    char msg[128];
    snprintf(msg, sizeof msg, "kernel of %d x %d: kernels are odd and at most %d x %d", kh, kw,
             kConvMaxKernel, kConvMaxKernel);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (kernel_stride != 0 && kernel_stride != kh * kw)
    return fail(BSGP_ERR_ARG, "kernel_stride must be 0 (one kernel) or kh * kw (one per image)");
  if (conv_tiles(H, W, kh, kw) > 0xffffffLL)  // workgroups of 256 threads: a grid below 2^32
    return fail(BSGP_ERR_UNSUPPORTED, "an image is covered by at most 2^24 - 1 tiles of 64 columns");
  ConvArgs a{};
  a.data = data, a.kernel = kernel, a.kernel_sum = kernel_sum, a.mask = mask;
  a.fill_value = fill_value, a.out = out, a.status = status_out;
  a.B = B, a.H = H, a.W = W, a.kh = kh, a.kw = kw, a.kernel_stride = kernel_stride;
  a.flags = flags;
  HIP_TRY(launch_convolve(a, dtype == BSGP_DTYPE_F32, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_detect_sources(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                        const double* threshold_map, double threshold, int32_t npixels,
                        int32_t connectivity, const uint8_t* mask, int32_t* labels_out,
                        int32_t* nlabels_out, void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!labels_out || !nlabels_out) return fail(BSGP_ERR_ARG, "labels_out / nlabels_out is NULL");
  if (int rc = check_dtype(dtype)) return rc;
  if (npixels < 1) return fail(BSGP_ERR_ARG, "npixels must be >= 1");
  if (connectivity != 4 && connectivity != 8)
    return fail(BSGP_ERR_ARG, "connectivity must be 4 or 8");
  if (int rc = seg_shape(B, H, W)) return rc;
  const size_t hw = (size_t)H * W;
  SegArgs a{};
  a.data = data, a.thr_map = threshold_map, a.mask = mask, a.thr = threshold;
  a.B = B, a.H = H, a.W = W, a.npixels = npixels, a.conn = connectivity;
  a.nblk = (int)((hw + kSegChunk - 1) / kSegChunk);
  a.labels_out = labels_out, a.nlabels_out = nlabels_out;
  hipStream_t s = (hipStream_t)stream;
  // stream-ordered workspace: the call stays asynchronous
  const size_t per = 2 * hw + (size_t)a.nblk;
  StreamScratch w(s);
  if (int rc = w.alloc((size_t)B * per * sizeof(int))) return rc;
  a.lab = static_cast<int*>(w.p);
  a.area = a.lab + (size_t)B * hw;
  a.blk = a.area + (size_t)B * hw;
  return w.finish(launch_seg_detect(a, dtype == BSGP_DTYPE_F32, s), "detection");
}

int bsgp_segment_catalog(const double* data, const double* conv, const int32_t* labels, int32_t B,
                         int32_t H, int32_t W, int32_t cap, const int32_t* nlabels,
                         int32_t* int_cols_out, double* f64_cols_out, int32_t* status_out,
                         void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!labels) return fail(BSGP_ERR_ARG, "labels is NULL");
  if (!int_cols_out || !f64_cols_out || !status_out)
    return fail(BSGP_ERR_ARG, "int_cols_out / f64_cols_out / status_out is NULL");
  if (cap < 1) return fail(BSGP_ERR_ARG, "cap must be >= 1");
  if (int rc = seg_shape(B, H, W)) return rc;
  SegCatArgs a{};
  a.data = data, a.conv = conv, a.labels = labels, a.nlabels = nlabels;
  a.B = B, a.H = H, a.W = W, a.cap = cap;
  a.icols = int_cols_out, a.fcols = f64_cols_out, a.status = status_out;
  HIP_TRY(launch_seg_catalog(a, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_segment_local_background(const void* data, int32_t dtype, const int32_t* labels, int32_t B,
                                  int32_t H, int32_t W, int32_t cap, const int32_t* nlabels,
                                  const int32_t* int_cols, double* f64_cols,
                                  double localbkg_width, double sigma, int32_t maxiters,
                                  int32_t min_pixels, int32_t apply, double* lb_out,
                                  int32_t* npix_out, int32_t* status_out, void* stream) {
  if (!(localbkg_width > 0.0) || !std::isfinite(localbkg_width))
    return fail(BSGP_ERR_ARG, "localbkg_width must be finite and > 0");
  if (!(sigma > 0.0)) return fail(BSGP_ERR_ARG, "sigma must be > 0");
  if (maxiters < 0) return fail(BSGP_ERR_ARG, "maxiters must be >= 0");
  if (min_pixels < 1) return fail(BSGP_ERR_ARG, "min_pixels must be >= 1");
  if (int rc = check_dtype(dtype)) return rc;
  if (cap < 1) return fail(BSGP_ERR_ARG, "cap must be >= 1");
  if (B == 0) return BSGP_OK;  // no image: nothing to do, no pointer is followed
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!labels || !int_cols) return fail(BSGP_ERR_ARG, "labels / int_cols is NULL");
  if (apply && !f64_cols) return fail(BSGP_ERR_ARG, "f64_cols is NULL (apply != 0)");
  if (!lb_out || !npix_out || !status_out)
    return fail(BSGP_ERR_ARG, "lb_out / npix_out / status_out is NULL");
  if (int rc = seg_shape(B, H, W)) return rc;
  LocalBkgArgs a{};
  a.data = data, a.labels = labels, a.nlabels = nlabels, a.icols = int_cols, a.fcols = f64_cols;
  a.B = B, a.H = H, a.W = W, a.cap = cap, a.maxiters = maxiters, a.min_pixels = min_pixels;
  a.apply = apply ? 1 : 0, a.width = localbkg_width, a.sigma = sigma;
  a.lb = lb_out, a.npix = npix_out, a.status = status_out;
  hipStream_t s = (hipStream_t)stream;
  const size_t rows = (size_t)B * cap;
  HIP_TRY(hipMemsetAsync(lb_out, 0, rows * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(npix_out, 0, 2 * rows * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(status_out, 0, (size_t)B * sizeof(int), s));
  HIP_TRY(launch_localbkg(a, dtype == BSGP_DTYPE_F32, s));
  return BSGP_OK;
}

// both deblending entry points; lds_max_box < 0: bsgp_deblend_sources (no global-memory path)
static int deblend_sources(const double* data, const int32_t* labels, int32_t B, int32_t H, int32_t W,
                           int32_t cap, const int32_t* nlabels, const int32_t* int_cols,
                           const uint8_t* select, int32_t npixels, int32_t nlevels, double contrast,
                           int32_t mode, int32_t connectivity, int32_t lds_max_box,
                           int32_t* labels_out, int32_t* nlabels_out, int32_t* status_out,
                           void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!labels || !nlabels || !int_cols) return fail(BSGP_ERR_ARG, "labels / nlabels / int_cols is NULL");
  if (!labels_out || !nlabels_out || !status_out)
    return fail(BSGP_ERR_ARG, "labels_out / nlabels_out / status_out is NULL");
  if (labels_out == labels) return fail(BSGP_ERR_ARG, "labels_out must not be labels");
  if (cap < 1) return fail(BSGP_ERR_ARG, "cap must be >= 1");
  if (npixels < 1) return fail(BSGP_ERR_ARG, "npixels must be >= 1");
  if (nlevels < 1) return fail(BSGP_ERR_ARG, "nlevels must be >= 1");
  if (!(contrast >= 0.0 && contrast <= 1.0)) return fail(BSGP_ERR_ARG, "contrast must lie in [0, 1]");
  if (mode != BSGP_DEBLEND_LINEAR && mode != BSGP_DEBLEND_EXPONENTIAL)
    return fail(BSGP_ERR_ARG, "mode must be BSGP_DEBLEND_LINEAR or BSGP_DEBLEND_EXPONENTIAL");
  if (connectivity != 4 && connectivity != 8)
    return fail(BSGP_ERR_ARG, "connectivity must be 4 or 8");
  if (int rc = seg_shape(B, H, W)) return rc;
  DeblendArgs a{};
  a.data = data, a.labels = labels, a.nlabels = nlabels, a.icols = int_cols, a.sel = select;
  a.B = B, a.H = H, a.W = W, a.cap = cap, a.npixels = npixels, a.nlevels = nlevels;
  a.conn = connectivity, a.mode = mode, a.contrast = contrast;
  a.labels_out = labels_out, a.nlabels_out = nlabels_out, a.status = status_out;
  a.large = lds_max_box >= 0;
  a.lds_max_box = a.large ? lds_max_box : kDeblendMaxBox;
  hipStream_t s = (hipStream_t)stream;
  // stream-ordered workspace: the call stays asynchronous.  The global-memory
  // path adds 32 bytes per pixel (one double and six ints), sized by B, H, W
  // alone and never initialised.
  const size_t rows = (size_t)B * cap, px = a.large ? (size_t)B * H * W : 0;
  StreamScratch w(s);
  if (int rc = w.alloc(px * (sizeof(double) + 6 * sizeof(int)) + 2 * rows * sizeof(int))) return rc;
  a.hkey = static_cast<double*>(w.p);
  a.lev = reinterpret_cast<int*>(a.hkey + px);
  a.reg = a.lev + px, a.cnt = a.reg + px, a.kept = a.cnt + px, a.mk = a.kept + px;
  a.hidx = a.mk + px;
  a.nchild = a.hidx + px;
  a.base = a.nchild + rows;
  hipError_t e = hipMemsetAsync(a.nchild, 0, rows * sizeof(int), s);
  if (e == hipSuccess) e = hipMemsetAsync(status_out, 0, (size_t)B * sizeof(int), s);
  if (e == hipSuccess) e = launch_deblend(a, s);
  return w.finish(e, "deblend");
}

int bsgp_deblend_sources(const double* data, const int32_t* labels, int32_t B, int32_t H, int32_t W,
                         int32_t cap, const int32_t* nlabels, const int32_t* int_cols,
                         const uint8_t* select, int32_t npixels, int32_t nlevels, double contrast,
                         int32_t mode, int32_t connectivity, int32_t* labels_out,
                         int32_t* nlabels_out, int32_t* status_out, void* stream) {
  return deblend_sources(data, labels, B, H, W, cap, nlabels, int_cols, select, npixels, nlevels,
                         contrast, mode, connectivity, -1, labels_out, nlabels_out, status_out,
                         stream);
}

int bsgp_deblend_sources_large(const double* data, const int32_t* labels, int32_t B, int32_t H,
                               int32_t W, int32_t cap, const int32_t* nlabels,
                               const int32_t* int_cols, const uint8_t* select, int32_t npixels,
                               int32_t nlevels, double contrast, int32_t mode,
                               int32_t connectivity, int32_t lds_max_box, int32_t* labels_out,
                               int32_t* nlabels_out, int32_t* status_out, void* stream) {
  if (lds_max_box < 0 || lds_max_box > BSGP_DEBLEND_MAX_BOX)
    return fail(BSGP_ERR_ARG, "lds_max_box must lie in 0 .. BSGP_DEBLEND_MAX_BOX");
  return deblend_sources(data, labels, B, H, W, cap, nlabels, int_cols, select, npixels, nlevels,
                         contrast, mode, connectivity, lds_max_box, labels_out, nlabels_out,
                         status_out, stream);
}

namespace {
// M2 on the host: the float64 after the largest one whose square root is <=
// max_sep.  sqrt is monotone and max_sep^2 is rounded once, so the walk from
// it takes a step or two.
double match_d2_limit(double max_sep) {
  double t = max_sep * max_sep;
  if (std::isinf(t)) t = std::numeric_limits<double>::max();
  while (t > 0.0 && std::sqrt(t) > max_sep) t = std::nextafter(t, 0.0);
  for (double u = std::nextafter(t, HUGE_VAL); std::isfinite(u) && std::sqrt(u) <= max_sep;
       u = std::nextafter(t, HUGE_VAL))
    t = u;
  return std::nextafter(t, HUGE_VAL);
}

// threads per workgroup of the match kernels: BSGP_MATCH_BLOCK (a multiple of 64
// in 64..1024; tools/match_timing.py's knob), else the fastest of 64 .. 1024 on
// every workload of profiles/match: 1024 in LDS, 512 in global memory
int match_block(bool lds, int rows) {
  int block = lds ? 1024 : 512;
  if (const char* e = getenv("BSGP_MATCH_BLOCK")) {
    const int v = atoi(e);
    if (v >= 64 && v <= 1024 && v % 64 == 0) block = v;
  }
  const int need = (rows + 63) / 64 * 64;  // no wave without a row
  return need < block ? need : block;
}
}  // namespace

int bsgp_match_catalogs(const double* x1, const double* y1, int32_t stride1, const int32_t* valid1,
                        int32_t vstride1, int32_t cap1, const int32_t* n1, const double* x2,
                        const double* y2, int32_t stride2, const int32_t* valid2, int32_t vstride2,
                        int32_t cap2, const int32_t* n2, int32_t B, double max_sep, int32_t path,
                        int32_t* match1_out, int32_t* match2_out, double* sep1_out,
                        int32_t* npairs_out, int32_t* status_out, void* stream) {
  if (!(max_sep >= 0.0) || !std::isfinite(max_sep))
    return fail(BSGP_ERR_ARG, "max_sep must be finite and >= 0");
  if (cap1 < 1 || cap2 < 1) return fail(BSGP_ERR_ARG, "cap1 and cap2 must be >= 1");
  if (B < 0) return fail(BSGP_ERR_ARG, "B must be >= 0");
  if (stride1 < 1 || stride2 < 1) return fail(BSGP_ERR_ARG, "stride1 and stride2 must be >= 1");
  if (path != BSGP_MATCH_AUTO && path != BSGP_MATCH_LDS && path != BSGP_MATCH_GLOBAL)
    return fail(BSGP_ERR_ARG, "path must be BSGP_MATCH_AUTO, BSGP_MATCH_LDS or BSGP_MATCH_GLOBAL");
  if (B == 0) return BSGP_OK;  // no image: nothing to do, no pointer is followed
  if (!x1 || !y1 || !x2 || !y2) return fail(BSGP_ERR_ARG, "x1 / y1 / x2 / y2 is NULL");
  if ((valid1 && vstride1 < 1) || (valid2 && vstride2 < 1))
    return fail(BSGP_ERR_ARG, "vstride1 and vstride2 must be >= 1 where valid is given");
  if (!match1_out || !match2_out || !sep1_out || !npairs_out || !status_out)
    return fail(BSGP_ERR_ARG,
                "match1_out / match2_out / sep1_out / npairs_out / status_out is NULL");
  char msg[160];
  if (cap1 > kMatchMax || cap2 > kMatchMax) {
    snprintf(msg, sizeof msg, "catalogues of %d and %d rows: a catalogue holds at most %d", cap1,
             cap2, kMatchMax);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  const bool fits = (int64_t)cap1 + cap2 <= kMatchLdsMax;
  if (path == BSGP_MATCH_LDS && !fits) {
    snprintf(msg, sizeof msg, "cap1 + cap2 = %d: the LDS path holds at most %d rows", cap1 + cap2,
             kMatchLdsMax);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  const bool lds = path == BSGP_MATCH_LDS || (path == BSGP_MATCH_AUTO && fits);
  MatchArgs a{};
  a.c1 = MatchCat{x1, y1, valid1, n1, stride1, valid1 ? vstride1 : 1, cap1};
  a.c2 = MatchCat{x2, y2, valid2, n2, stride2, valid2 ? vstride2 : 1, cap2};
  a.d2_lim = match_d2_limit(max_sep);
  a.match1 = match1_out, a.match2 = match2_out, a.sep1 = sep1_out;
  a.npairs = npairs_out, a.status = status_out;
  hipStream_t s = (hipStream_t)stream;
  const int rows = match_rows(cap1, cap2), block = match_block(lds, rows);
  if (lds) {
    HIP_TRY(launch_match(a, B, true, block, s));
    return BSGP_OK;
  }
  // stream-ordered workspace: the call stays asynchronous
  StreamScratch w(s);
  if (int rc = w.alloc((size_t)B * rows * kMatchRowBytes)) return rc;
  a.ws_xy = static_cast<double*>(w.p);
  a.ws_state = reinterpret_cast<int*>(a.ws_xy + (size_t)B * rows * 2);
  return w.finish(launch_match(a, B, false, block, s), "match");
}

int bsgp_radial_profile(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                        const double* centers, int32_t rcap, double* prof, int32_t* len,
                        void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!centers) return fail(BSGP_ERR_ARG, "centers is NULL");
  if (!prof || !len) return fail(BSGP_ERR_ARG, "prof / len is NULL");
  if (int rc = check_dtype(dtype)) return rc;
  if (B < 1 || H < 1 || W < 1) return fail(BSGP_ERR_ARG, "B, H and W must be >= 1");
  if (rcap < 1) return fail(BSGP_ERR_ARG, "rcap must be >= 1");
  char msg[160];
  if ((int64_t)H * W > kStampMaxPixels) {
    snprintf(msg, sizeof msg, "stamp of %lld pixels: a stamp holds at most %d (H * W <= %d)",
             (long long)H * W, kStampMaxPixels, kStampMaxPixels);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (rcap > kStampMaxBins) {
    snprintf(msg, sizeof msg, "%d radial bins: a profile holds at most %d", rcap, kStampMaxBins);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  StampProfArgs a{};
  a.data = data, a.centers = centers, a.B = B, a.H = H, a.W = W, a.rcap = rcap;
  a.prof = prof, a.len = len;
  HIP_TRY(launch_stamp_radprof(a, dtype == BSGP_DTYPE_F32, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_fit_gauss1d(const double* prof, const int32_t* len, int32_t B, int32_t rcap,
                     const double* fwhm, double* fitted, double* params, double* perr,
                     int32_t* info, void* stream) {
  if (!prof || !len || !fwhm) return fail(BSGP_ERR_ARG, "prof / len / fwhm is NULL");
  if (!fitted || !params || !perr || !info)
    return fail(BSGP_ERR_ARG, "fitted / params / perr / info is NULL");
  if (B < 1 || rcap < 1) return fail(BSGP_ERR_ARG, "B and rcap must be >= 1");
  if (rcap > kStampMaxBins) {
    char msg[128];
    snprintf(msg, sizeof msg, "profiles of %d values: a profile holds at most %d", rcap,
             kStampMaxBins);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  StampFitArgs a{};
  a.prof = prof, a.len = len, a.fwhm = fwhm, a.B = B, a.rcap = rcap;
  a.fitted = fitted, a.params = params, a.perr = perr, a.info = info;
  HIP_TRY(launch_stamp_fit(a, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_wasserstein1(const double* u, const int32_t* ulen, const double* v, const int32_t* vlen,
                      int32_t B, int32_t rcap, double* out, void* stream) {
  if (!u || !v) return fail(BSGP_ERR_ARG, "u / v is NULL");
  if (!out) return fail(BSGP_ERR_ARG, "out is NULL");
  if (B < 1 || rcap < 1) return fail(BSGP_ERR_ARG, "B and rcap must be >= 1");
  if (rcap > kStampMaxBins) {
    char msg[128];
    snprintf(msg, sizeof msg, "samples of %d values: a sample holds at most %d", rcap,
             kStampMaxBins);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  StampW1Args a{};
  a.u = u, a.v = v, a.ulen = ulen, a.vlen = vlen, a.B = B, a.rcap = rcap, a.out = out;
  a.P = 2;
  while (a.P < 2 * rcap) a.P *= 2;
  HIP_TRY(launch_stamp_w1(a, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_extract_stamps(const void* img, int32_t dtype, int32_t H, int32_t W, const double* xy,
                        int32_t n, int32_t sh, int32_t sw, void* out, int32_t* box_out,
                        int32_t* status_out, void* stream) {
  if (n < 0) return fail(BSGP_ERR_ARG, "n must be >= 0");
  if (int rc = check_dtype(dtype)) return rc;
  if (H < 1 || W < 1) return fail(BSGP_ERR_ARG, "H and W must be >= 1");
  if (sh < 1 || sw < 1) return fail(BSGP_ERR_ARG, "the stamp size (sh, sw) must be >= 1");
  if ((int64_t)sh * sw > kStampCutMaxPixels) {
    char msg[128];
    snprintf(msg, sizeof msg, "stamp of %lld pixels: a cutout holds at most %d",
             (long long)sh * sw, kStampCutMaxPixels);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (n == 0) return BSGP_OK;
  if (!img) return fail(BSGP_ERR_ARG, "img is NULL");
  if (!xy) return fail(BSGP_ERR_ARG, "xy is NULL");
  if (!out || !box_out || !status_out)
    return fail(BSGP_ERR_ARG, "out / box_out / status_out is NULL");
  StampCutArgs a{};
  a.img = img, a.xy = xy, a.H = H, a.W = W, a.n = n, a.sh = sh, a.sw = sw;
  a.out = out, a.box = box_out, a.status = status_out;
  HIP_TRY(launch_extract_stamps(a, dtype == BSGP_DTYPE_F32, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_stamp_select(const int32_t* res_nlabels, const double* res_cols, int32_t res_stride,
                      const double* obs_cols, int32_t obs_stride, const int32_t* iters, int32_t n,
                      int32_t K, double* scores_out, int32_t* best_out, double* rows_out,
                      int32_t* num_iters_out, int32_t* status_out, void* stream) {
  if (n < 0) return fail(BSGP_ERR_ARG, "n must be >= 0");
  if (K < 1) return fail(BSGP_ERR_ARG, "K must be >= 1");
  if (res_stride < 8 || obs_stride < 8)
    return fail(BSGP_ERR_ARG, "res_stride and obs_stride must be >= 8");
  if ((int64_t)n * K > 0x7fffffff) return fail(BSGP_ERR_ARG, "n * K must be below 2^31");
  if (n == 0) return BSGP_OK;
  if (!res_nlabels || !res_cols || !obs_cols || !iters)
    return fail(BSGP_ERR_ARG, "res_nlabels / res_cols / obs_cols / iters is NULL");
  if (!scores_out || !best_out || !rows_out || !num_iters_out || !status_out)
    return fail(BSGP_ERR_ARG,
                "scores_out / best_out / rows_out / num_iters_out / status_out is NULL");
  StampSelectArgs a{};
  a.res_nlabels = res_nlabels, a.res_cols = res_cols, a.obs_cols = obs_cols, a.iters = iters;
  a.n = n, a.K = K, a.res_stride = res_stride, a.obs_stride = obs_stride;
  a.scores = scores_out, a.best = best_out, a.rows = rows_out, a.num_iters = num_iters_out;
  a.status = status_out;
  HIP_TRY(launch_stamp_select(a, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_validate_sources(const void* image, int32_t dtype, const double* bkgmap,
                          const double* rmsmap, int32_t B, int32_t H, int32_t W,
                          int32_t maps_per_image, const double* xy, int32_t xy_stride,
                          const int32_t* n, int32_t cap, int32_t sh, int32_t sw, double nsigma,
                          double* stats_out, int32_t* valid_out, int32_t* status_out,
                          void* stream) {
  if (B < 0 || cap < 0) return fail(BSGP_ERR_ARG, "B and cap must be >= 0");
  if (int rc = check_dtype(dtype)) return rc;
  if (H < 1 || W < 1) return fail(BSGP_ERR_ARG, "H and W must be >= 1");
  if (sh < 1 || sw < 1) return fail(BSGP_ERR_ARG, "the window size (sh, sw) must be >= 1");
  if (xy_stride < 2) return fail(BSGP_ERR_ARG, "xy_stride must be >= 2");
  if (std::isnan(nsigma)) return fail(BSGP_ERR_ARG, "nsigma is NaN");
  if ((int64_t)sh * sw > kValidateMax) {
    char msg[128];
    snprintf(msg, sizeof msg, "window of %lld values: a validation window holds at most %d",
             (long long)sh * sw, kValidateMax);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (B == 0 || cap == 0) return BSGP_OK;
  if (int rc = seg_shape(B, H, W)) return rc;
  if (!image || !bkgmap || !rmsmap) return fail(BSGP_ERR_ARG, "image / bkgmap / rmsmap is NULL");
  if (!xy) return fail(BSGP_ERR_ARG, "xy is NULL");
  if (!stats_out || !valid_out || !status_out)
    return fail(BSGP_ERR_ARG, "stats_out / valid_out / status_out is NULL");
  ValidateArgs a{};
  a.img = image, a.bkg = bkgmap, a.rms = rmsmap, a.xy = xy, a.n = n;
  a.B = B, a.H = H, a.W = W, a.maps_per_image = maps_per_image ? 1 : 0, a.xy_stride = xy_stride;
  a.cap = cap, a.sh = sh, a.sw = sw, a.nsigma = nsigma;
  a.stats = stats_out, a.valid = valid_out, a.status = status_out;
  hipStream_t s = (hipStream_t)stream;
  const size_t rows = (size_t)B * cap;
  // rows beyond an image's count: NaN statistics (all bits set), valid 0, status 0
  HIP_TRY(hipMemsetAsync(stats_out, 0xff, 3 * rows * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(valid_out, 0, rows * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(status_out, 0, rows * sizeof(int), s));
  HIP_TRY(launch_validate(a, dtype == BSGP_DTYPE_F32, s));
  return BSGP_OK;
}

namespace {
// the shape header of a fit from the caller's model, its sizes checked
int psffit_shape(const bsgp_psf_model* m, int32_t B, int32_t cap, PsfShape* out) {
  if (B < 0 || cap < 0) return fail(BSGP_ERR_ARG, "B and cap must be >= 0");
  if (!m) return fail(BSGP_ERR_ARG, "model is NULL");
  if (m->hw < 0 || m->hw > 255 || m->ngauss < 1 || m->ldeg < 0 || m->sdeg < 0)
    return fail(BSGP_ERR_ARG, "bad PSF model degrees or half width");
  const int64_t ncomp = (int64_t)m->ngauss * (m->ldeg + 1) * (m->ldeg + 2) / 2;
  const int64_t nterm = (int64_t)(m->sdeg + 1) * (m->sdeg + 2) / 2;
  if (m->ngauss > kPsfFitMaxCoef || m->ldeg > kPsfFitMaxCoef || m->sdeg > kPsfFitMaxCoef ||
      ncomp * nterm > kPsfFitMaxCoef) {
    char msg[128];
    snprintf(msg, sizeof msg, "a model of %lld coefficients: a fit holds at most %d",
             (long long)(ncomp * nterm), kPsfFitMaxCoef);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (cap > kPsfFitMaxStars) {
    char msg[128];
    snprintf(msg, sizeof msg, "%d stars: a frame holds at most %d", cap, kPsfFitMaxStars);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (B > 65535) return fail(BSGP_ERR_UNSUPPORTED, "B must be at most 65535");
  PsfShape s{};
  s.cosv = m->cos, s.sinv = m->sin, s.ax = m->ax, s.ay = m->ay;
  s.sig2 = m->sigma_inc * m->sigma_inc;
  s.x_orig = m->x_orig, s.y_orig = m->y_orig;
  s.ngauss = m->ngauss, s.ldeg = m->ldeg, s.sdeg = m->sdeg, s.hw = m->hw;
  s.ncomp = (int)ncomp, s.nterm = (int)nterm;
  *out = s;
  return BSGP_OK;
}
}  // namespace

int bsgp_psf_fit_moments(const void* image, int32_t dtype, int32_t B, int32_t H, int32_t W,
                         const double* xy, const int32_t* n, int32_t cap,
                         const bsgp_psf_model* model, double fitrad, const double* flux,
                         const double* sky, int32_t sky_mode, const uint8_t* mask, int32_t has_sat,
                         double sat_level, double* G_out, double* h_out, double* vv_out,
                         int32_t* npix_out, double* flux_out, int32_t* status_out, void* stream) {
  PsfFitMomentArgs a{};
  if (int rc = psffit_shape(model, B, cap, &a.shape)) return rc;
  if (int rc = check_dtype(dtype)) return rc;
  if (H < 1 || W < 1) return fail(BSGP_ERR_ARG, "H and W must be >= 1");
  if (!(fitrad > 0.0)) return fail(BSGP_ERR_ARG, "fitrad must be > 0");
  if (sky_mode < 0 || sky_mode > 2) return fail(BSGP_ERR_ARG, "sky_mode must be 0, 1 or 2");
  if (B == 0 || cap == 0) return BSGP_OK;
  if (int rc = seg_shape(B, H, W)) return rc;
  if (!image || !xy) return fail(BSGP_ERR_ARG, "image / xy is NULL");
  if (sky_mode != 0 && !sky) return fail(BSGP_ERR_ARG, "sky is NULL");
  if (!G_out || !h_out || !vv_out || !npix_out || !flux_out || !status_out)
    return fail(BSGP_ERR_ARG, "G_out / h_out / vv_out / npix_out / flux_out / status_out is NULL");
  a.img = image, a.xy = xy, a.n = n, a.flux = flux, a.sky = sky_mode ? sky : nullptr, a.mask = mask;
  a.B = B, a.H = H, a.W = W, a.cap = cap, a.sky_mode = sky_mode, a.has_sat = has_sat ? 1 : 0;
  a.fitrad2 = fitrad * fitrad, a.sat_level = sat_level;
  a.G = G_out, a.h = h_out, a.vv = vv_out, a.flux_out = flux_out, a.npix = npix_out;
  a.status = status_out;
  hipStream_t s = (hipStream_t)stream;
  const size_t rows = (size_t)B * cap, nc = a.shape.ncomp;
  HIP_TRY(hipMemsetAsync(G_out, 0, rows * (nc * (nc + 1) / 2) * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(h_out, 0, rows * nc * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(vv_out, 0, rows * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(flux_out, 0, rows * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(npix_out, 0, rows * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(status_out, 0, rows * sizeof(int), s));
  HIP_TRY(launch_psffit_moments(a, dtype == BSGP_DTYPE_F32, s));
  return BSGP_OK;
}

int bsgp_psf_fit_solve(int32_t B, int32_t cap, const int32_t* n, const double* xy,
                       const bsgp_psf_model* model, const double* G, const double* h,
                       const double* vv, const int32_t* npix, const int32_t* mstatus,
                       const double* weights, int32_t niter, double nsig, int32_t min_stars,
                       double* coef_out, int32_t* used_out, int32_t* status_out, double* rms_out,
                       int32_t* frame_out, void* stream) {
  PsfFitSolveArgs a{};
  if (int rc = psffit_shape(model, B, cap, &a.shape)) return rc;
  if (niter < 0 || min_stars < 0) return fail(BSGP_ERR_ARG, "niter and min_stars must be >= 0");
  if (std::isnan(nsig)) return fail(BSGP_ERR_ARG, "nsig is NaN");
  if (B == 0 || cap == 0) return BSGP_OK;
  if (!xy || !G || !h || !vv || !npix || !mstatus)
    return fail(BSGP_ERR_ARG, "xy / G / h / vv / npix / mstatus is NULL");
  if (!coef_out || !used_out || !status_out || !rms_out || !frame_out)
    return fail(BSGP_ERR_ARG, "coef_out / used_out / status_out / rms_out / frame_out is NULL");
  a.xy = xy, a.n = n, a.G = G, a.h = h, a.vv = vv, a.npix = npix, a.mstatus = mstatus;
  a.weights = weights;
  a.B = B, a.cap = cap, a.niter = niter, a.min_stars = min_stars, a.nsig = nsig;
  a.coef = coef_out, a.rms = rms_out, a.used = used_out, a.status = status_out;
  a.frame = frame_out;
  hipStream_t s = (hipStream_t)stream;
  // rows beyond a frame's count: status 0, rms NaN (all bits set)
  HIP_TRY(hipMemsetAsync(status_out, 0, (size_t)B * cap * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(rms_out, 0xff, (size_t)B * cap * sizeof(double), s));
  HIP_TRY(launch_psffit_solve(a, s));
  return BSGP_OK;
}

namespace {
// the support of a star template from the caller's half widths, checked
int star_support(const int32_t* halfw, int32_t R, signed char* out, int* n) {
  if (R < 0) return fail(BSGP_ERR_ARG, "R must be >= 0");
  if (R > kStarMaxR) {
    char msg[128];
    snprintf(msg, sizeof msg, "a support of R = %d: a star template reaches at most %d pixels", R,
             kStarMaxR);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (!halfw) return fail(BSGP_ERR_ARG, "halfw is NULL");
  int cnt = 0;
  for (int r = 0; r <= 2 * R; ++r) {
    if (halfw[r] < 0 || halfw[r] > R) return fail(BSGP_ERR_ARG, "halfw must lie in 0..R");
    out[r] = (signed char)halfw[r];
    cnt += 2 * halfw[r] + 1;
  }
  *n = cnt;
  return BSGP_OK;
}

int star_template(const double* tmpl, const int32_t* halfw, int32_t R, double tt,
                  StarTemplate* tp) {
  if (int rc = star_support(halfw, R, tp->halfw, &tp->n)) return rc;
  if (!tmpl) return fail(BSGP_ERR_ARG, "tmpl is NULL");
  if (!(tt > 0.0) || !std::isfinite(tt)) return fail(BSGP_ERR_ARG, "tt must be finite and > 0");
  tp->t = tmpl, tp->R = R, tp->tt = tt, tp->sqrt_tt = std::sqrt(tt);
  return BSGP_OK;
}
}  // namespace

int bsgp_star_maps(const void* image, int32_t dtype, int32_t B, int32_t H, int32_t W,
                   const uint8_t* mask, const double* tmpl, const int32_t* halfw, int32_t R,
                   double tt, double* corr_out, double* amp_out, void* stream) {
  StarMapArgs a{};
  if (int rc = star_template(tmpl, halfw, R, tt, &a.tp)) return rc;
  if (int rc = check_dtype(dtype)) return rc;
  if (int rc = seg_shape(B, H, W)) return rc;
  if (!image || !corr_out || !amp_out)
    return fail(BSGP_ERR_ARG, "image / corr_out / amp_out is NULL");
  a.data = image, a.mask = mask, a.B = B, a.H = H, a.W = W, a.corr = corr_out, a.amp = amp_out;
  HIP_TRY(launch_star_maps(a, dtype == BSGP_DTYPE_F32, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_star_peaks(const void* image, int32_t dtype, int32_t B, int32_t H, int32_t W,
                    const double* corr, const double* amp, const double* tmpl,
                    const int32_t* halfw, int32_t R, double tt, const double* noise,
                    int32_t noise_is_map, double c_min, double thresh, int32_t peak_hw,
                    int32_t cap, int32_t* peaks_out, int32_t* n_out, int32_t* status_out,
                    void* stream) {
  StarPeakArgs a{};
  if (int rc = star_template(tmpl, halfw, R, tt, &a.tp)) return rc;
  if (int rc = check_dtype(dtype)) return rc;
  if (int rc = seg_shape(B, H, W)) return rc;
  if (peak_hw < 0 || peak_hw > 3) return fail(BSGP_ERR_ARG, "peak_hw must lie in 0..3");
  if (cap < 1) return fail(BSGP_ERR_ARG, "cap must be >= 1");
  if (cap > kStarMax) {
    char msg[128];
    snprintf(msg, sizeof msg, "%d stars: a frame holds at most %d", cap, kStarMax);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (std::isnan(c_min) || std::isnan(thresh)) return fail(BSGP_ERR_ARG, "c_min / thresh is NaN");
  if (!image || !corr || !amp || !noise)
    return fail(BSGP_ERR_ARG, "image / corr / amp / noise is NULL");
  if (!peaks_out || !n_out || !status_out)
    return fail(BSGP_ERR_ARG, "peaks_out / n_out / status_out is NULL");
  a.data = image, a.corr = corr, a.amp = amp, a.noise = noise;
  a.B = B, a.H = H, a.W = W, a.noise_map = noise_is_map ? 1 : 0, a.peak_hw = peak_hw, a.cap = cap;
  a.nblk = (int)(((int64_t)H * W + kStarChunk - 1) / kStarChunk);
  a.c_min = c_min, a.thresh = thresh;
  a.peaks = peaks_out, a.n = n_out, a.status = status_out;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(peaks_out, 0, (size_t)B * cap * 2 * sizeof(int), s));
  // stream-ordered workspace: the call stays asynchronous
  StreamScratch w(s);
  const size_t chunks = (size_t)B * a.nblk;
  if (int rc = w.alloc(chunks * sizeof(int) + chunks * 256)) return rc;
  a.blk = static_cast<int*>(w.p);
  a.flag = reinterpret_cast<unsigned char*>(a.blk + chunks);
  return w.finish(launch_star_peaks(a, dtype == BSGP_DTYPE_F32, s), "star peaks");
}

int bsgp_star_measure(const void* image, int32_t dtype, int32_t B, int32_t H, int32_t W,
                      const uint8_t* mask, const double* corr, const double* amp,
                      const int32_t* halfw, int32_t R, const int32_t* peaks, const int32_t* n,
                      int32_t cap, double anrad1, double anrad2, int32_t bkg_alg, double sigma,
                      int32_t maxiters, int32_t min_sky, int32_t has_sat, double sat_level,
                      double dxy, double* fcols_out, int32_t* icols_out, void* stream) {
  StarMeasureArgs a{};
  int nsup = 0;
  if (int rc = star_support(halfw, R, a.halfw, &nsup)) return rc;
  if (int rc = check_dtype(dtype)) return rc;
  if (int rc = seg_shape(B, H, W)) return rc;
  if (cap < 1) return fail(BSGP_ERR_ARG, "cap must be >= 1");
  if (cap > kStarMax) return fail(BSGP_ERR_UNSUPPORTED, "cap is above BSGP_STARFIND_MAX");
  if (!(anrad1 >= 0.0) || !(anrad1 < anrad2) || !std::isfinite(anrad2))
    return fail(BSGP_ERR_ARG, "the annulus needs 0 <= anrad1 < anrad2");
  if (anrad2 >= (double)(kStarMaxBox + 1))
    return fail(BSGP_ERR_UNSUPPORTED, "anrad2 must be below 1025");
  if (bkg_alg < BSGP_STARFIND_BKG_MODE || bkg_alg > BSGP_STARFIND_BKG_MEAN)
    return fail(BSGP_ERR_ARG, "bkg_alg must be BSGP_STARFIND_BKG_MODE, _MEDIAN or _MEAN");
  if (maxiters < 0 || min_sky < 1)
    return fail(BSGP_ERR_ARG, "maxiters must be >= 0, min_sky >= 1");
  if (std::isnan(sigma) || std::isnan(dxy) || (has_sat && std::isnan(sat_level)))
    return fail(BSGP_ERR_ARG, "sigma / dxy / sat_level is NaN");
  if (!image || !corr || !amp || !peaks || !n)
    return fail(BSGP_ERR_ARG, "image / corr / amp / peaks / n is NULL");
  if (!fcols_out || !icols_out) return fail(BSGP_ERR_ARG, "fcols_out / icols_out is NULL");
  a.data = image, a.mask = mask, a.corr = corr, a.amp = amp, a.peaks = peaks, a.n = n;
  a.B = B, a.H = H, a.W = W, a.cap = cap, a.R = R, a.box = (int)std::floor(anrad2);
  a.bkg_alg = bkg_alg, a.maxiters = maxiters, a.min_sky = min_sky, a.has_sat = has_sat ? 1 : 0;
  a.r1sq = anrad1 * anrad1, a.r2sq = anrad2 * anrad2, a.sigma = sigma, a.sat_level = sat_level;
  a.dxy2 = dxy * dxy;
  a.fcols = fcols_out, a.icols = icols_out;
  hipStream_t s = (hipStream_t)stream;
  // rows beyond a frame's count: NaN columns (all bits set), zero integers
  HIP_TRY(hipMemsetAsync(fcols_out, 0xff, (size_t)B * cap * 8 * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(icols_out, 0, (size_t)B * cap * 4 * sizeof(int), s));
  HIP_TRY(launch_star_measure(a, dtype == BSGP_DTYPE_F32, s));
  return BSGP_OK;
}

int bsgp_star_select(const double* fcols, const int32_t* icols, const int32_t* n, int32_t B,
                     int32_t cap, int32_t H, int32_t W, int32_t hw, double min_flux,
                     int32_t has_max_peak, double max_peak, double rat_thresh,
                     double iso_radius, int32_t npsf_max, int32_t* eligible_out,
                     int32_t* rank_out, int32_t* selected_out, void* stream) {
  if (B < 0 || cap < 0) return fail(BSGP_ERR_ARG, "B and cap must be >= 0");
  if (H < 1 || W < 1) return fail(BSGP_ERR_ARG, "H and W must be >= 1");
  if (hw < 0 || npsf_max < 0) return fail(BSGP_ERR_ARG, "hw and npsf_max must be >= 0");
  if (std::isnan(min_flux) || std::isnan(rat_thresh) || std::isnan(iso_radius) ||
      (has_max_peak && std::isnan(max_peak)))
    return fail(BSGP_ERR_ARG, "min_flux / max_peak / rat_thresh / iso_radius is NaN");
  if (cap > kStarMax) return fail(BSGP_ERR_UNSUPPORTED, "cap is above BSGP_STARFIND_MAX");
  if (B > 65535) return fail(BSGP_ERR_UNSUPPORTED, "B must be at most 65535");
  if (B == 0 || cap == 0) return BSGP_OK;
  if (!fcols || !icols) return fail(BSGP_ERR_ARG, "fcols / icols is NULL");
  if (!eligible_out || !rank_out || !selected_out)
    return fail(BSGP_ERR_ARG, "eligible_out / rank_out / selected_out is NULL");
  StarSelectArgs a{};
  a.fcols = fcols, a.icols = icols, a.n = n;
  a.B = B, a.cap = cap, a.H = H, a.W = W, a.hw = hw, a.has_max_peak = has_max_peak ? 1 : 0;
  a.npsf_max = npsf_max, a.min_flux = min_flux, a.max_peak = max_peak;
  a.rat_thresh = rat_thresh, a.iso2 = iso_radius * iso_radius;
  a.eligible = eligible_out, a.rank = rank_out, a.selected = selected_out;
  hipStream_t s = (hipStream_t)stream;
  const size_t rows = (size_t)B * cap;
  HIP_TRY(hipMemsetAsync(eligible_out, 0, rows * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(rank_out, 0xff, rows * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(selected_out, 0, rows * sizeof(int), s));
  HIP_TRY(launch_star_select(a, s));
  return BSGP_OK;
}

int bsgp_beta_div(int64_t n, const double* y, const double* x, double beta, double* out,
                  void* stream) {
  if (n < 1 || n > 0x7fffffff || !y || !x || !out) return fail(BSGP_ERR_ARG, "bad arguments");
  HIP_TRY(launch_beta_div((int)n, y, x, beta, out, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_beta_div_deriv(int64_t n, const double* y, const double* x, double beta, double* out,
                        void* stream) {
  if (n < 1 || !y || !x || !out) return fail(BSGP_ERR_ARG, "bad arguments");
  HIP_TRY(launch_beta_div_deriv(n, y, x, beta, out, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_beta_div_grad_parts(int64_t n, const double* den, const double* gn, double beta,
                             double* pow1, double* w, void* stream) {
  if (n < 1 || !den || !gn || !pow1 || !w) return fail(BSGP_ERR_ARG, "bad arguments");
  HIP_TRY(launch_grad_parts(n, den, gn, beta, pow1, w, (hipStream_t)stream));
  return BSGP_OK;
}

}  // extern "C"
