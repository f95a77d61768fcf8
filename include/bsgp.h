/* bsgp.h — C ABI of the MI355X beta-SGP engine (libbsgp.so, gfx950).
 *
 * The reference boundary is a Python API, not an FFI: restoration/sgp.py's
 * sgp() (sgp.py:41-47), sgp_betaDiv() (sgp.py:506-513), the betaDiv family
 * (sgp.py:441-503) and flux_conserve_proj.projectDF() (flux_conserve_proj.py:7).
 * The drop-in Python modules beta-sgp_amd/sgp.py and
 * beta-sgp_amd/flux_conserve_proj.py keep those signatures and bind the entry
 * points below through ctypes (INTEGRATION.md shows the stubs).
 *
 * Conventions
 *  - plain C types only; device pointers are HBM buffers of the calling
 *    process's current HIP device; `stream` is a hipStream_t passed as void*
 *    (NULL = the null stream). Entry points are asynchronous on `stream`
 *    unless their comment says otherwise.
 *  - every function returns BSGP_OK (0) or a negative status; the message of
 *    the last failure on the calling thread is in bsgp_last_error().
 *  - all arrays are C-contiguous little-endian float64; an image batch is
 *    [B][H][W].
 *  - a plan is not thread-safe: one plan per device per host thread.
 */
#ifndef BSGP_H_
#define BSGP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSGP_OK 0
#define BSGP_ERR_ARG (-1)          /* bad argument / shape                       */
#define BSGP_ERR_HIP (-2)          /* a HIP runtime call failed                  */
#define BSGP_ERR_UNSUPPORTED (-3)  /* geometry the kernels do not cover (yet)    */
#define BSGP_ERR_PSF (-4)          /* PSF not normalised (sgp.py:97-102)         */

/* conv_mode: which A/AT the solver uses.
 *  BSGP_CONV_CIRCULAR    use_original_SGP_Afunction=True  (sgp.py:108-120):
 *                        A(x)=Re ifft2(fft2(fftshift(psf)) . fft2(x)), AT uses conj;
 *                        psf must have the image's shape.
 *  BSGP_CONV_LINEAR_FILL use_original_SGP_Afunction=False (sgp.py:121-161):
 *                        astropy convolve_fft(x, psf/sum(psf)) with zero fill,
 *                        cropped; AT convolves with psf.T. */
#define BSGP_CONV_CIRCULAR 0
#define BSGP_CONV_LINEAR_FILL 1

#define BSGP_VARIANT_KL 0   /* sgp()          sgp.py:41-438  */
#define BSGP_VARIANT_BETA 1 /* sgp_betaDiv()  sgp.py:506-895 */

typedef struct bsgp_plan_s* bsgp_plan;

/* Every keyword argument of sgp()/sgp_betaDiv() that reaches the iteration.
 * Field meanings are the reference's (sgp.py:48-77, 515-542). */
typedef struct {
  int32_t variant;        /* BSGP_VARIANT_*                                        */
  int32_t init_recon;     /* 0 zeros, 1 x0 given (randn, sgp.py:169-170), 2 gn, 3 flat */
  int32_t proj_type;      /* 0 clamp at 0, 1 flux-conserving projectDF             */
  int32_t stop_criterion; /* 0/1 MAXIT only, 2 step norm, 3 rel. decrease, 4 discrepancy */
  int32_t MAXIT;
  int32_t M_alpha;        /* <= 32 */
  int32_t M;              /* <= 32 */
  int32_t max_projs;
  double gamma, beta, alpha, alpha_min, alpha_max, tau;
  double ccd_sat_level;   /* used when has_sat */
  double betaParam, lr, lr_exp_param;
  double tol_convergence;
  double prescaled_scaling; /* scale_data == 2: the scaling the caller applied    */
  double prescaled_tol4;    /* scale_data == 2 and stop_criterion 4: 1+1/mean(gn) */
  int32_t has_sat;
  int32_t scale_data;     /* 0 none, 1 scaling = max(gn) on device (sgp.py:193-199),
                             2 inputs already scaled by the caller in their own dtype:
                             gn, bkg, x0 are used as given (x0 required); with
                             gn_f32, 0 and 1 run the float32 prelude on the device
                             (see below)                                           */
  int32_t verbose;        /* only changes tol**2 for stop_criterion 2 (sgp.py:291-294) */
  int32_t adapt_beta;
  int32_t schedule_lr;
  int32_t bkg_is_map;     /* bkg is [B][H][W] instead of [B] scalars               */
  int32_t ls_spec;        /* line-search lambdas evaluated per pass (1..8); 1 when adapt_beta */
  int32_t ls_series;      /* 1: small trial steps from the moment series (general beta) */
  int32_t streams;        /* sub-batches run on this many streams (1..16: the caller's + 15 plan
                             streams) so phases overlap; more than GPU_MAX_HW_QUEUES share queues */
  int32_t team;           /* workgroups cooperating on one image: 0 = auto (spread the
                             batch over the CUs when B is small), 1 = one per image,
                             k > 1 = at most k (capped so every workgroup is resident) */
  int32_t proj_cache;     /* 1: projectDF evaluations whose multiplier falls inside a
                             bracket known to hold the root read only the pixels that
                             change state inside it (a per-lane list written by the
                             last full pass); 0: every evaluation streams the image */
  int32_t gn_compact;     /* 1: an image whose observed values are all finite and exact
                             in f32 (counts, or f32 FITS data) keeps them in f32 and
                             recomputes the scaled gn/scaling (and the null-pixel fill)
                             on every read, bit-identical to f64 storage; the line
                             search reads half the bytes of gn. 0: f64 storage */
  int32_t gn_f32;         /* 1: gn is the reference's float32 image (scale_data == 2: the
                             caller scaled it in float32).  Under numpy 1.x promotion the
                             beta objective then sums s*gn**beta as float32 terms
                             (exponent rounded to float32) with numpy's float32 pairwise
                             reduction, and rounds (s*beta)*gn to float32 before the
                             multiply by den**(beta-1) (sgp.py:457-458); the device
                             reproduces both.  With proj_type 0 the first iteration's
                             scaling matrix clips to float32 bounds (sgp.py:726-729). */
  int32_t beta0_general;  /* 1: every in->beta0[b] is neither 0 nor 1, so a batch with
                             per-image betas can use the general-beta kernels */
  int32_t flux_f32;       /* gn_f32 with scale_data 0/1: in->flux holds numpy float32
                             values, divided by the scaling in float32 (sgp.py:666) */
  int32_t persistent;     /* 1: one-workgroup images (team 1, per-wave transforms, no
                             err / x_iter) run every iteration in ONE persistent launch
                             that dequeues (iteration, image) tasks; the same device
                             code per iteration, bit-identical results.  0: one launch
                             per phase and iteration on sub-batch streams */
} bsgp_params;
/* gn_f32 with scale_data 0 or 1 (ABI 3): the float32 prelude of sgp.py:620-666
 * runs on the device.  in->gn holds the raw float32 image values (exact in
 * float64), in->bkg float64 backgrounds, in->flux the raw provided flux; the
 * device takes scaling = max(gn), gn/scaling and (init_recon 2) x/scaling in
 * float32, the null-pixel fill rounded to float32, stop rule 4's 1 + 1/mean(gn)
 * from numpy's float32 mean, and init_recon 3's flat start rounded to float32,
 * as numpy 1.x evaluates them for a float32 image (bkg/scaling, a float64
 * flux/scaling and x0/scaling stay float64).  Not covered (the caller scales):
 * float32 backgrounds, and init_recon 3 without a flux and with a scalar bkg
 * (numpy sums that start in float32). */

/* Storage of the per-image iteration vectors (bsgp_plan_create). */
#define BSGP_STORAGE_F64 0
#define BSGP_STORAGE_F32 1

/* Device inputs of a batched solve. */
typedef struct {
  const double* gn;    /* [B][H][W] observed images (any scale; scaled on device) */
  const double* bkg;   /* [B] or [B][H][W] (bkg_is_map)                           */
  const double* flux;  /* [B] precomputed flux or NULL = sum(gn - bkg); unscaled, or
                          already scaled when scale_data == 2 (sgp.py:208-211)      */
  const double* x0;    /* [B][H][W] initial x (init_recon == 1, or scale_data == 2), else NULL */
  const double* beta0; /* [B] per-image initial betaParam or NULL = params.betaParam */
  const double* obj;   /* [B][H][W] ground truth (unscaled) for out->err, or NULL  */
} bsgp_inputs;

/* Device outputs of a batched solve.  MAXIT1 = MAXIT + 1. */
typedef struct {
  double* x;           /* [B][H][W] restored image (x * scaling)                  */
  int32_t* iters;      /* [B] iterations (the reference's returned iter_)         */
  double* discr;       /* [B][MAXIT1] discrepancy 2/N*scaling*f (sgp.py:276,392)  */
  double* times;       /* [B][MAXIT1] seconds since solve start (sgp.py:391), may be NULL */
  double* crit;        /* [B][MAXIT1] stop-rule value per iteration, may be NULL  */
  int32_t* flags;      /* [B][MAXIT1] bit0: fv >= fr warning (sgp.py:351, 803);
                          bits 8..23: line-search trials of iteration k (the
                          betaDiv calls of sgp.py:782 / objective evaluations of
                          :334 in iteration k); may be NULL */
  double* beta_final;  /* [B] final betaParam (sgp.py:892), may be NULL           */
  int64_t* counters;   /* [B][8]: proj evals E_p, line-search trials E_ls,
                          line-search passes over the image, status bits (1: line
                          search cap, 4: team barrier timed out, 8: no positive
                          entry in flux/(flux+bkg)*AT(gn), where the reference
                          raises, sgp.py:269-270), trials evaluated
                          from the small-step series, team size T, projection
                          passes over the image, projection-list entries read;
                          may be NULL */
  double* err;         /* [B][MAXIT1] relative error ||x_k - obj|| / ||obj|| of the
                          scaled iterate after the initial projection (k = 0) and after
                          iteration k (errflag, sgp.py:240-257, 394-396); needs in->obj;
                          may be NULL */
  double* x_iter;      /* [B][MAXIT][H][W] the scaled iterate after each iteration,
                          before the revert (save=True writes these, sgp.py:416-422);
                          may be NULL */
} bsgp_outputs;

/* Plan: geometry, FFT sizes, twiddles and the PSF transfer functions for A and
 * AT, built on the device from the host PSF [kh][kw].  storage: BSGP_STORAGE_F64,
 * or BSGP_STORAGE_F32 (iteration vectors kept in float32 in HBM, every sum and
 * scalar in float64; SURVEY config C4).  Synchronous. */
int bsgp_plan_create(int32_t H, int32_t W, const double* psf_host, int32_t kh, int32_t kw,
                     int32_t conv_mode, int32_t storage, int32_t device, bsgp_plan* out);
/* The same; psf_checked != 0 skips the normalisation check because the caller
 * has applied the reference's check (sgp.py:97-102 / 557-562: np.sum in the
 * PSF's OWN dtype) before widening the PSF to float64 -- a float32 PSF whose
 * float32 sum is 1 has a float64 sum off by up to ~1e-7, which the float64
 * check here would refuse.  The Python drop-in always checks first. */
int bsgp_plan_create_checked(int32_t H, int32_t W, const double* psf_host, int32_t kh,
                             int32_t kw, int32_t conv_mode, int32_t storage, int32_t device,
                             int32_t psf_checked, bsgp_plan* out);
int bsgp_plan_destroy(bsgp_plan plan);
/* FFT grid (P x Q) and the per-slot workspace bytes of the plan. */
int bsgp_plan_info(bsgp_plan plan, int32_t* P, int32_t* Q, int64_t* slot_bytes,
                   int32_t* fft_waves);

/* Batched SGP / beta-SGP: B independent images (or (image, beta) candidates),
 * each solved to completion by one persistent workgroup. Asynchronous. */
int bsgp_solve_device(bsgp_plan plan, int32_t B, const bsgp_params* params,
                      const bsgp_inputs* in, const bsgp_outputs* out, void* stream);

/* Measurement: bsgp_solve_device on the one stream `stream` (params->streams is
 * taken as 1) with a HIP event recorded around every kernel launch;
 * kernel_ms[k] and launches[k] (k < 6) receive the summed span and the launch
 * count of kernel class k: 0 setup, 1 k_dir, 2 k_col (A and AT), 3 k_ls, 4 k_bb,
 * 5 k_persist (the persistent solver: every iteration in one launch).
 * Synchronous (waits for the solve). */
int bsgp_solve_profiled(bsgp_plan plan, int32_t B, const bsgp_params* params,
                        const bsgp_inputs* in, const bsgp_outputs* out, void* stream,
                        double* kernel_ms, int64_t* launches);

/* Same with host buffers (copies in, solves, copies out). Synchronous. */
int bsgp_solve_host(bsgp_plan plan, int32_t B, const bsgp_params* params,
                    const bsgp_inputs* in, const bsgp_outputs* out);

/* A (transpose=0) or AT (transpose=1) of the plan on B images. Asynchronous.
 * Replaces the partial(afunction/A/AT, ...) operators of sgp.py:119-120,160-161. */
int bsgp_apply_operator(bsgp_plan plan, int32_t B, int32_t transpose, const double* x,
                        double* out, void* stream);

/* flux_conserve_proj.projectDF(b, c, dia, scaling, ccd_sat_level, lambda_,
 * dlambda_, tol_lam, biter, siter, max_projs) on one vector of length n.
 * x: output [n]; info: output [4] = {final lambda, evaluations, biter, siter}.
 * Asynchronous. */
int bsgp_project_df(int64_t n, double b, const double* c, const double* dia, double scaling,
                    int32_t has_sat, double ccd_sat_level, double lambda0, double dlambda0,
                    double tol_lam, int32_t biter, int32_t siter, int32_t max_projs, double* x,
                    double* info, void* stream);

/* betaDiv(y, x, beta) (sgp.py:441-458) -> out[0]. Asynchronous. */
int bsgp_beta_div(int64_t n, const double* y, const double* x, double beta, double* out,
                  void* stream);
/* betaDivDeriv(y, x, beta) elementwise (sgp.py:462-495) -> out[n]. Asynchronous. */
int bsgp_beta_div_deriv(int64_t n, const double* y, const double* x, double beta, double* out,
                        void* stream);
/* The two elementwise parts of betaDivDerivwrtY (sgp.py:498-499):
 * pow1 = den**(beta-1), w = gn*den**(beta-2). Asynchronous. */
int bsgp_beta_div_grad_parts(int64_t n, const double* den, const double* gn, double beta,
                             double* pow1, double* w, void* stream);

/* ---- data paths either side of the solver ---------- */

/* Overlapping subdivision tiles of an [H][W] field: out[t] = img[y0:y1, x0:x1]
 * for boxes[t] = {x0, y0, x1, y1} (device int32 [n][4], xyxy as
 * restoration/utils.py:332-372 calculate_slice_bboxes returns them), every
 * box exactly th x tw and inside the field.  Replaces create_subdivisions'
 * Cutout2D cutouts (utils.py:375-386).  Asynchronous. */
int bsgp_extract_tiles(const double* img, int32_t H, int32_t W, const int32_t* boxes, int32_t n,
                       int32_t th, int32_t tw, double* out, void* stream);

/* Mean co-add of n th x tw tiles at boxes into an [H][W] mosaic; footprint
 * (may be NULL) = number of tiles covering each pixel; uncovered pixels are 0.
 * Tiles are summed in index order (deterministic).  The same-WCS case of
 * reproject_and_coadd (utils.py:389-395) with combine_function='mean' and no
 * background matching (bsgp_coadd_tiles_matched below has it).  n <= 8192.
 * Asynchronous. */
int bsgp_coadd_tiles(const double* tiles, int32_t n, int32_t th, int32_t tw, const int32_t* boxes,
                     int32_t H, int32_t W, double* mean, double* footprint, void* stream);

/* ---- background-matched co-add --------------------
 * reproject_and_coadd(..., match_background=True) for tiles on one pixel grid
 * (restoration/utils.py:392-397), in three asynchronous steps whose arguments
 * all live on the device.  The pairs of overlapping tiles, their adjacency
 * lists and the connected components (B1) are integer geometry of the boxes
 * and come from the caller (beta-sgp_amd/subdivisions.py tile_pairs).
 * n <= 8192 as for bsgp_coadd_tiles; th * tw < 2^31. */
#define BSGP_COADD_NONFINITE 1      /* a pair of this tile held a non-finite difference: dropped */
#define BSGP_COADD_ISOLATED 2       /* no pair (left): correction 0                              */
#define BSGP_COADD_NOT_CONVERGED 4  /* the solver stopped at its iteration cap                   */

/* B2 (utils.py:392-397): offsets[p] = numpy.median(tile_i - tile_j) over the
 * intersection of boxes i and j for pairs[p] = {i, j}, i < j (int32
 * [npairs][2]); bit-equal to numpy.median (the middle value of an odd count,
 * (lo + hi) / 2 of the two middle values of an even one).  A pair whose overlap
 * holds a non-finite difference gets NaN, which drops it from the graph, and
 * BSGP_COADD_NONFINITE in status of both tiles; so does a pair that does not
 * intersect, without the bit.  status (int32 [n]) is zeroed first.  npairs may
 * be 0.  Asynchronous. */
int bsgp_tile_offsets(const double* tiles, int32_t n, int32_t th, int32_t tw, const int32_t* boxes,
                      const int32_t* pairs, int32_t npairs, double* offsets, int32_t* status,
                      void* stream);

/* B3 (utils.py:392-397): corrections = the minimum-norm least-squares solution
 * of c_i - c_j = O_ij over the pairs with a finite offset, the fixed point of
 * reproject's solve_corrections_sgd: conjugate gradients on the graph Laplacian
 * from c = 0 in one workgroup, float64, fixed-order sums (deterministic), down
 * to a relative residual of 1e-13 or n iterations (BSGP_COADD_NOT_CONVERGED in
 * every status word); zero mean within every connected component; a tile
 * without a pair gets 0 and BSGP_COADD_ISOLATED.  Row i's neighbours are
 * nbr[row_ptr[i] .. row_ptr[i + 1]), nbr_pair the index of that pair in
 * offsets, nbr_sign +1 where i is the pair's first tile (O_ij = offsets[pair])
 * and -1 where it is the second; component [n] in 0 .. ncomp - 1.
 * background_reference >= 0: c -= c[background_reference] afterwards; < 0: none.
 * Bits are added to status (the one bsgp_tile_offsets wrote, or zeros).
 * solve_info (may be NULL): {iterations, relative residual reached}.
 * Asynchronous. */
int bsgp_tile_corrections(int32_t n, const int32_t* row_ptr, const int32_t* nbr,
                          const int32_t* nbr_pair, const int32_t* nbr_sign,
                          const int32_t* component, int32_t ncomp, const double* offsets,
                          int32_t background_reference, double* corrections, int32_t* status,
                          double* solve_info, void* stream);

/* B4 (utils.py:392-397): bsgp_coadd_tiles with corrections[t] taken off every
 * value of tile t before it is added: mean = sum_t (tile_t - c_t) / count in
 * tile order; the footprint is bsgp_coadd_tiles'.  n <= 8192.  Asynchronous. */
int bsgp_coadd_tiles_matched(const double* tiles, int32_t n, int32_t th, int32_t tw,
                             const int32_t* boxes, const double* corrections, int32_t H, int32_t W,
                             double* mean, double* footprint, void* stream);

/* FITS primary-array samples (big-endian, BITPIX 8/16/32/64/-32/-64) to f64:
 * out[i] = BZERO + BSCALE * sample[i] (FITS standard 4.0 §5.3; IEEE samples
 * exact).  raw: device copy of the data block, 8-byte aligned.  Replaces
 * astropy.io.fits reads of the results/ and psf/ FITS files.  Asynchronous. */
int bsgp_fits_to_f64(const void* raw, int64_t n, int32_t bitpix, double bscale, double bzero,
                     double* out, void* stream);

/* Sky background of B images [B][H][W] on the device: the estimator
 * restoration/utils.py:235-239 builds with photutils, Background2D(data,
 * box_size, filter_size, bkg_estimator=MedianBackground()) with its default
 * SigmaClip(sigma, maxiters), exclude_percentile and pad-and-mask edges,
 * restated from astropy.stats.SigmaClip and scipy.ndimage:
 * per bh x bw box the sigma-clipped median and population std of its valid
 * pixels (inside the image, finite, mask byte 0); boxes with more than
 * exclude_percentile/100 * bh*bw invalid pixels are filled from the 10 nearest
 * kept cells (inverse distance); both meshes are median-filtered over fh x fw
 * cells (odd, <= 7) and zoomed by cubic B-spline to [H][W], clamped to the
 * filtered mesh's range if clip.
 *   data        device, float32 or float64 (dtype = BSGP_DTYPE_*), widened to
 *               float64 before any arithmetic
 *   mask        device bytes [B][H][W], nonzero = masked, or NULL
 *   bkg_out, rms_out            [B][H][W] maps
 *   mesh_out, rms_mesh_out      [B][ny][nx] filtered meshes, ny = ceil(H/bh)
 *   medians_out                 [B][2] medians of the two filtered meshes
 *   status_out  int32 [B][1 + 3*ny*nx]: the number of kept boxes (0: every box
 *               was excluded and the image's outputs are NaN), then per cell
 *               the excluded flag, the pixels that survived clipping and the
 *               clipping iterations run
 * Every output pointer may be NULL.  bh*bw <= 4096 and ny*nx <= 4096, else
 * BSGP_ERR_UNSUPPORTED.  Asynchronous (stream-ordered workspace). */
#define BSGP_DTYPE_F32 0
#define BSGP_DTYPE_F64 1
int bsgp_background2d(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t bh,
                      int32_t bw, int32_t fh, int32_t fw, double sigma, int32_t maxiters,
                      double exclude_percentile, int32_t clip, const uint8_t* mask, double* bkg_out,
                      double* rms_out, double* mesh_out, double* rms_mesh_out, double* medians_out,
                      int32_t* status_out, void* stream);

/* DIAPL PSF model: the values of a psf*.bin.txt coefficient file
 * (psf/psf_calculate.py:10-47 reads them in this order) plus the degrees the
 * reference evaluates with (ldeg = 2, sdeg = 1: psf_calculate.py:24-25). */
typedef struct {
  int32_t hw;            /* stamp half width: stamps are (2hw+1) x (2hw+1)  (value 0) */
  int32_t ngauss;        /* Gaussian components                           (value 3) */
  int32_t ldeg;          /* local polynomial degree of calc_psf_pix (self.ldeg) */
  int32_t sdeg;          /* spatial polynomial degree of init_psf (self.sdeg) */
  double cos, sin;       /* values 5-6 */
  double ax, ay;         /* values 7-8 */
  double sigma_inc;      /* value 9 */
  double x_orig, y_orig; /* values 12-13: origin of the spatial expansion */
  const double* coeffs;  /* host: values 14.. (ngauss*(ldeg+1)(ldeg+2)/2 per spatial term) */
  int32_t ncoef;
} bsgp_psf_model;

/* n PSF stamps [n][2hw+1][2hw+1] (device out).  spatial = 0: the local
 * coefficients are coeffs[0:ncomp] for every stamp (get_psf_mat,
 * psf_calculate.py:89-107; xy may be NULL); spatial = 1: the coefficients at
 * field position xy[2i], xy[2i+1] (device, (x, y)) by the spatial expansion of
 * init_psf (:140-165).  normalize = 1 divides each stamp by its numpy-order sum
 * (normalize_psf_mat, :129-137).  Pixel (r, c) is calc_psf_pix(x = c - hw,
 * y = r - hw) (:98-103).  Asynchronous. */
int bsgp_psf_stamps(const bsgp_psf_model* model, const double* xy, int32_t n, int32_t spatial,
                    int32_t normalize, double* out, void* stream);

/* Per-image PSFs: replace the plan's transfer functions with n pairs built on
 * the device from device PSF stamps [n][kh][kw] (the kh x kw the plan was
 * created with; H x W in circular mode), each checked like sgp.py:97-102.
 * Afterwards bsgp_solve_* and bsgp_apply_operator on this plan need B == n and
 * image i is convolved with PSF i (the spatially varying PSF of each
 * subdivision).  Synchronous. */
int bsgp_plan_set_psfs(bsgp_plan plan, const double* psfs_dev, int32_t n, void* stream);

/* ---- solver state: save after a solve, resume later --------- */

/* One fixed-size record per image, self-contained: a resume needs a plan of
 * the same geometry and storage, the parameters and the records, not the
 * original inputs.  A record is BSGP_STATE_HEADER_BYTES of header (the struct
 * below, zero padded) followed by the sections of bsgp_state_layout, every
 * section starting on a 16-byte boundary and zero padded to the next:
 *   discr, crit, times  float64[hist_cap]   the outputs' rows 0..iters_done
 *   flags               int32[hist_cap]
 *   x, g, x_tf, pw      V[N], N = H*W, V = the plan's storage type: the iterate
 *                       after iteration iters_done, its gradient, A(x) and
 *                       den^(beta-1) (beta objective; unused for KL).  An image
 *                       that a stop rule stopped holds the iterate it returned
 *                       (sgp.py:424-438: the one before its last iteration).
 *   gn                  float64[N]: the slot's scaled observed image verbatim
 *                       (g32 != 0: the raw float32 values in its first half)
 *   bkg                 float64[N] scaled background map (bkg_is_map only)
 * The direction transform d_tf, the spectrum, the projection pixel lists and
 * the team partials are rebuilt by every iteration and are not stored. */
#define BSGP_STATE_MAGIC 0x53475342u /* "BSGS" */
#define BSGP_STATE_VERSION 1
#define BSGP_STATE_HEADER_BYTES 1024

typedef struct {
  uint32_t magic;        /* BSGP_STATE_MAGIC                                       */
  uint32_t version;      /* BSGP_STATE_VERSION (layout version)                    */
  int32_t H, W;
  int32_t storage;       /* BSGP_STORAGE_*                                         */
  int32_t conv_mode;     /* BSGP_CONV_*                                            */
  int32_t hist_cap;      /* rows of the history sections (> iters_done)            */
  int32_t T;             /* team size of the solve (counters[:, 5])                */
  int32_t iters_done;    /* iterations completed                                   */
  int32_t stopped;       /* 0: goes on when resumed (it ran out of MAXIT only);
                            1: a stop rule (or a timeout, status bit 4) ended it;
                            8: the setup ended it (status bit 8)                   */
  int32_t Xones;         /* scaling matrix still ones (init_recon 0, no iteration) */
  int32_t epoch;         /* lr_schedule's epoch (sgp.py:766-767)                   */
  int32_t g32;           /* compact gn: 0 float64, 1 raw float32, 2 raw / scaling  */
  int32_t beta0_given;   /* the solve had per-image betas (in->beta0)              */
  int64_t record_bytes;  /* bytes of this record (bsgp_state_layout offs[0])       */
  int64_t counters[7];   /* cumulative: E_p, E_ls, line-search passes, status bits,
                            series trials, projection passes, list entries read    */
  double scaling, flux, bkg_scalar; /* scaled flux; scaled scalar background       */
  double x_low, x_upp;   /* scaling-matrix bounds (sgp.py:268-273)                 */
  double Dcoeff, tol;    /* 2/N*scaling; the stop rule's tolerance                 */
  double elapsed;        /* seconds of solve time so far (times continue from it)  */
  double fv, alpha, tau, lr, init_lr, beta;
  double lam_p, lam_ratio, kappa; /* projection multiplier history (proj_cache)    */
  double konst;          /* lambda-independent objective sum at `beta`             */
  double gfill;          /* null-pixel fill of a compact gn                        */
  double Valpha[32];     /* first M_alpha entries used                             */
  double Fold[32];       /* first M entries used                                   */
  bsgp_params prm;       /* the parameters of the solve (validated on resume)      */
} bsgp_state_header;

/* Byte offsets inside a record for a geometry (no plan, no device needed):
 * offs[0] = record bytes, then the offsets of discr, crit, times, flags, x, g,
 * x_tf, pw, gn, bkg (offs[10] = 0 without a background map). */
int bsgp_state_layout(int32_t H, int32_t W, int32_t storage, int32_t bkg_is_map,
                      int32_t hist_cap, int64_t* offs /* [11] */);
/* Record bytes for a plan and a history of MAXIT_done_max + 1 rows. */
int bsgp_state_bytes(bsgp_plan plan, int32_t bkg_is_map, int32_t MAXIT_done_max,
                     int64_t* bytes_per_image);
/* Gather the state the last bsgp_solve_device / bsgp_solve_resume on this plan
 * left in its workspace into state_dev: B records of bytes_per_image =
 * bsgp_state_bytes(plan, bkg_is_map, MAXIT) each.  B is that solve's B; its
 * output buffers must still be valid (their discr / crit / times / flags rows
 * are the history; stop rule 2 needs out->crit), and no other solve may have
 * run on the plan in between.  Asynchronous. */
int bsgp_state_save(bsgp_plan plan, int32_t B, void* state_dev, int64_t bytes_per_image,
                    void* stream);
/* Continue B images from records up to params->MAXIT.  state_dev holds n_state
 * records of bytes_per_image; image i of this solve is record index[i] (device
 * int32 [B]) or record i (index NULL, B <= n_state).  The plan's geometry, mode
 * and storage, the team size and every numerical parameter must be the
 * record's (BSGP_ERR_ARG names the field that differs); MAXIT must exceed the
 * iterations done; streams, persistent, proj_cache and ls_spec may differ.
 * Outputs are those of the unsplit solve, bit for bit (times excepted), with
 * complete history rows; images whose record is stopped keep their results.
 * out->err / out->x_iter: BSGP_ERR_UNSUPPORTED.  Reads the record headers on
 * the host first (one stream synchronisation), then asynchronous. */
int bsgp_solve_resume(bsgp_plan plan, int32_t B, const bsgp_params* params,
                      const void* state_dev, int32_t n_state, int64_t bytes_per_image,
                      const int32_t* index, const bsgp_outputs* out, void* stream);

/* Source detection, deblending and segment measurement: what
 * utils.source_info (restoration/utils.py:235-247) does with photutils.
 * All of them are asynchronous; images of a batch are processed on their own and
 * get the bits they get alone; H * W < 2^31 and B <= 65535, else
 * BSGP_ERR_UNSUPPORTED.
 *
 * bsgp_convolve2d: astropy.convolution.convolve(data, kernel) with its
 * defaults on finite input (utils.py:242: boundary='fill', fill_value=0,
 * normalize_kernel=True).  out = (sum_i sum_j P[y+i][x+j] * K[kh-1-i][kw-1-j])
 * / sum(K), P the zero-padded input, every product rounded, rows outer, one
 * division by numpy's sum of the kernel.  kernel: device float64 [kh][kw],
 * odd and at most 7 x 7 (else BSGP_ERR_UNSUPPORTED).  data: float32 or float64
 * (dtype), widened first; out: float64 [B][H][W]; H <= 65535. */
int bsgp_convolve2d(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                    const double* kernel, int32_t kh, int32_t kw, double* out, void* stream);
/* bsgp_convolve2d_ex: astropy.convolution.convolve(array, kernel,
 * boundary='fill', fill_value, nan_treatment, normalize_kernel, mask,
 * preserve_nan) for kernels the size of a PSF (utils.py:46-56 degrade,
 * :249-272 scale_psf).  The sum is bsgp_convolve2d's: per output
 * pixel the taps run in row-major order of the window, tap (i, j) times
 * K[kh-1-i][kw-1-j], every product and sum rounded; a tap outside the image
 * contributes fill_value * k.
 *   kernel: device float64 [kh][kw] (kernel_stride 0, one for all images) or
 *   [B][kh][kw] (kernel_stride kh * kw, image b with kernel b); kh and kw odd
 *   and at most BSGP_CONV_MAX_KERNEL (else BSGP_ERR_UNSUPPORTED).
 *   kernel_sum: device float64 [1] or [B]: numpy's sum of each kernel, which
 *   the caller computes (it is not restated on the device).
 *   mask: uint8 [B][H][W], nonzero = masked (treated as NaN), or NULL.
 *   flags: BSGP_CONV_F_FILL replaces NaN and masked pixels by fill_value first
 *   (nan_treatment='fill'); without it (BSGP_CONV_F_INTERPOLATE) an image that
 *   holds a NaN or masked pixel takes, at every pixel, top / bot over the taps
 *   whose value is not NaN (bot: the sum of their kernel entries, same order),
 *   or data[y][x] where bot == 0, times kernel_sum without
 *   BSGP_CONV_F_NORMALIZE.  Every other image: top / kernel_sum with
 *   BSGP_CONV_F_NORMALIZE, else top.  BSGP_CONV_F_PRESERVE_NAN: NaN wherever
 *   the input was NaN or masked.  Infinities are values.
 *   fill_value must be finite.  data: float32 or float64 (dtype), widened
 *   first; out: float64 [B][H][W].
 *   status_out: device int32 [B]: BSGP_CONV_HAD_NAN the image held a NaN or a
 *   masked pixel, BSGP_CONV_NAN_LEFT some output is NaN that
 *   BSGP_CONV_F_PRESERVE_NAN did not put there.
 * Asynchronous; no host synchronisation. */
#define BSGP_CONV_MAX_KERNEL 63
#define BSGP_CONV_F_INTERPOLATE 0
#define BSGP_CONV_F_FILL 1
#define BSGP_CONV_F_NORMALIZE 2
#define BSGP_CONV_F_PRESERVE_NAN 4
#define BSGP_CONV_HAD_NAN 1
#define BSGP_CONV_NAN_LEFT 2
int bsgp_convolve2d_ex(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                       const double* kernel, int32_t kh, int32_t kw, int32_t kernel_stride,
                       const double* kernel_sum, const uint8_t* mask, int32_t flags,
                       double fill_value, double* out, int32_t* status_out, void* stream);
/* photutils' detect_sources (utils.py:243): a pixel is detected where data >
 * threshold (threshold_map [B][H][W] float64, or the scalar when it is NULL),
 * both finite and mask (bytes, nonzero = masked, or NULL) clear.  Components of
 * connectivity 8 or 4 with fewer than npixels pixels are removed; the others
 * are numbered 1..n by their first pixel in raster order (scipy.ndimage.label
 * and a consecutive relabel).  labels_out: int32 [B][H][W], 0 = background;
 * nlabels_out: int32 [B] on the device. */
int bsgp_detect_sources(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                        const double* threshold_map, double threshold, int32_t npixels,
                        int32_t connectivity, const uint8_t* mask, int32_t* labels_out,
                        int32_t* nlabels_out, void* stream);
/* The columns of photutils' SourceCatalog (utils.py:245-247) that need the
 * pixels, per label 1..min(cap, nlabels[b]) of image b (nlabels: device int32
 * [B], or NULL for cap): int_cols_out [B][cap][5] = area, bbox xmin, xmax,
 * ymin, ymax (inclusive); f64_cols_out [B][cap][8] = segment_flux, min_value,
 * max_value (of data), xcentroid, ycentroid, covar_sigx2, covar_sigxy,
 * covar_sigy2 (moments of conv, or of data when conv is NULL).  Rows beyond
 * an image's labels, and of labels it does not hold, have area 0 and zero
 * float columns.
 * status_out [B]: bit 0 nlabels[b] > cap, bit 1 a label outside
 * 1..min(cap, nlabels[b]) was met; such labels are skipped, never written. */
int bsgp_segment_catalog(const double* data, const double* conv, const int32_t* labels, int32_t B,
                         int32_t H, int32_t W, int32_t cap, const int32_t* nlabels,
                         int32_t* int_cols_out, double* f64_cols_out, int32_t* status_out,
                         void* stream);
/* The local background of photutils' SourceCatalog(..., localbkg_width=L)
 * (utils.py:244-246), modelled on photutils and pinned to the catalogue the
 * reference published for its frame.  For label l with inclusive box x0..x1,
 * y0..y1 (the int columns of bsgp_segment_catalog), w = x1 - x0 + 1,
 * h = y1 - y0 + 1 and L = localbkg_width > 0:
 *  L1 centre cx = (x0 + x1) / 2, cy = (y0 + y1) / 2; inner half-widths 0.75 w
 *     and 0.75 h; outer half-widths inner + L.
 *  L2 pixel (x, y) belongs to the annulus if |x - cx| < outer_x and
 *     |y - cy| < outer_y, not both |x - cx| < inner_x and |y - cy| < inner_y,
 *     it lies inside the image, and its label is 0 (pixels of any segment are
 *     left out, not only those of l).  Every comparison is strict.  Its value
 *     in data must be finite; values are widened to float64.
 *  L3 fewer than min_pixels (photutils: 10) values give a local background of
 *     0.0 and BSGP_LOCALBKG_FEW.
 *  L4 sigma clipping, astropy SigmaClip(sigma, maxiters, cenfunc='median',
 *     stdfunc='std') as bsgp_background2d does it: the values are sorted once,
 *     clipping moves the two ends of the sorted range, the bounds median -+
 *     sigma * std are inclusive, std is the population standard deviation.
 *     photutils uses sigma = 3, maxiters = 10.
 *  L5 SExtractor's mode of the survivors from their mean, median and
 *     population std: std == 0 gives mean; |mean - median| / std < 0.3 gives
 *     2.5 median - 1.5 mean; anything else gives median.
 *  L6 with apply != 0, in float64 with one rounding per operation:
 *     segment_flux -= area * lb, min_value -= lb, max_value -= lb (columns 0,
 *     1, 2 of f64_cols, rewritten in place).  The other columns are untouched.
 * data: float32 or float64 (dtype); labels, cap, nlabels, int_cols [B][cap][5]
 * and f64_cols [B][cap][8] as bsgp_segment_catalog takes and writes them
 * (f64_cols may be NULL when apply == 0).  lb_out: float64 [B][cap];
 * npix_out: int32 [B][cap][2] = values gathered, survivors of the clipping.
 * Rows beyond an image's labels and rows of area 0 get zeros.  An annulus of
 * more than BSGP_LOCALBKG_MAX values gets lb = 0, no correction and
 * BSGP_LOCALBKG_OVER_CAP.  status_out [B]: the OR over the image's labels.
 * Sums run over the sorted values, so a batch gives each image the bits it
 * gets alone.  B == 0 is a no-op that follows no pointer.  Asynchronous.
 * BSGP_ERR_ARG: localbkg_width not finite or <= 0, sigma not > 0, maxiters < 0,
 * min_pixels < 1, cap < 1, B < 0, a NULL array; the shape limits of
 * bsgp_segment_catalog give BSGP_ERR_UNSUPPORTED. */
#define BSGP_LOCALBKG_MAX 8192
#define BSGP_LOCALBKG_FEW 1
#define BSGP_LOCALBKG_OVER_CAP 2
int bsgp_segment_local_background(const void* data, int32_t dtype, const int32_t* labels, int32_t B,
                                  int32_t H, int32_t W, int32_t cap, const int32_t* nlabels,
                                  const int32_t* int_cols, double* f64_cols,
                                  double localbkg_width, double sigma, int32_t maxiters,
                                  int32_t min_pixels, int32_t apply, double* lb_out,
                                  int32_t* npix_out, int32_t* status_out, void* stream);

/* What SourceFinder(npixels, deblend=True) (utils.py:235, called at :242) adds to
 * detect_sources: photutils' deblend_sources, modelled on its documentation and
 * pinned to scipy.ndimage.label and skimage.segmentation.watershed.  Per
 * parent segment of labels (pixel set M, v = data on M):
 *  D1 smin, smax, ssum = sum v; smin == smax leaves the parent as it is.
 *  D2 thresholds k = 1..nlevels: linear smin + (smax - smin) / (nlevels + 1) * k;
 *     exponential m * (smax / m)^(k / (nlevels + 1)), m = smin, or 0.01 smax when
 *     smin == 0; exponential with smin < 0 uses linear.
 *  D3 per level, rising: the components of {p in M : v_p > t_k} with the given
 *     connectivity, those of fewer than npixels pixels dropped.
 *  D4 the regions start as {M}; a region holding two or more of a level's
 *     components is replaced by them; {M} after the last level leaves the
 *     parent.  The regions are the markers; a marker's identity is its first
 *     pixel in raster order.
 *  D5 watershed(-v, markers, mask=M): a priority queue keyed by (-v, index)
 *     (ties: the smaller index first; skimage: insertion age) holds the marker
 *     pixels; the smallest key is popped, and each unlabelled neighbour in M
 *     takes the popped pixel's label and is entered.
 *  D6 while a child has sum(v over it) / ssum < contrast, the child with the
 *     smallest fraction (tie: the smaller marker identity) is cleared and the
 *     flood repeated from the other children's full regions; fewer than two
 *     children leave the parent.
 *  D7 output labels 1..n: the parents left as they are first, in input order,
 *     then the children by parent, in marker order.
 * A pixel of M the flood cannot reach (connectivity 4 inside an 8-connected
 * parent) becomes 0, as the watershed leaves it.
 * data: float64 [B][H][W] (source_info passes the convolved image); labels:
 * int32 [B][H][W]; cap, nlabels [B] and int_cols [B][cap][5] as
 * bsgp_segment_catalog takes and writes them; select: bytes [B][cap], nonzero =
 * deblend this label, or NULL for all.  A parent with area < 2 npixels cannot
 * split and is skipped.  A parent whose bounding box holds more than
 * BSGP_DEBLEND_MAX_BOX pixels is left as it is and sets BSGP_DEBLEND_OVER_CAP in
 * status_out[b]; a label outside 0..min(cap, nlabels[b]) becomes 0 and sets
 * BSGP_DEBLEND_BAD_LABEL.  labels_out (int32 [B][H][W], not labels itself),
 * nlabels_out [B] and status_out [B] are written on the device.
 * BSGP_ERR_ARG: nlevels < 1, contrast outside [0, 1], npixels < 1, connectivity
 * not 4 or 8, an unknown mode. */
#define BSGP_DEBLEND_MAX_BOX 4096
#define BSGP_DEBLEND_LINEAR 0
#define BSGP_DEBLEND_EXPONENTIAL 1
#define BSGP_DEBLEND_OVER_CAP 1
#define BSGP_DEBLEND_BAD_LABEL 2
int bsgp_deblend_sources(const double* data, const int32_t* labels, int32_t B, int32_t H, int32_t W,
                         int32_t cap, const int32_t* nlabels, const int32_t* int_cols,
                         const uint8_t* select, int32_t npixels, int32_t nlevels, double contrast,
                         int32_t mode, int32_t connectivity, int32_t* labels_out,
                         int32_t* nlabels_out, int32_t* status_out, void* stream);
/* bsgp_deblend_sources with a second path for the parents it leaves: a parent
 * whose box holds at most lds_max_box pixels (0 .. BSGP_DEBLEND_MAX_BOX, else
 * BSGP_ERR_ARG) is deblended in LDS as above; every other parent by a kernel
 * that keeps its working set in global memory (one workgroup per parent, the
 * same steps D1 to D7, identities, orders and arithmetic, so a parent gets the
 * same labels from either path; lds_max_box = 0 sends every parent through the
 * global path).  Only a parent of more than BSGP_DEBLEND_LARGE_MAX_AREA pixels
 * is left as it is and sets BSGP_DEBLEND_OVER_CAP: its flood runs on one lane,
 * and the bound keeps that lane's work bounded.  The workspace, 32 bytes per
 * pixel of the batch, is stream-ordered and depends on B, H and
 * W only; the call stays asynchronous.  Everything else as
 * bsgp_deblend_sources. */
#define BSGP_DEBLEND_LARGE_MAX_AREA 262144
int bsgp_deblend_sources_large(const double* data, const int32_t* labels, int32_t B, int32_t H,
                               int32_t W, int32_t cap, const int32_t* nlabels,
                               const int32_t* int_cols, const uint8_t* select, int32_t npixels,
                               int32_t nlevels, double contrast, int32_t mode,
                               int32_t connectivity, int32_t lds_max_box, int32_t* labels_out,
                               int32_t* nlabels_out, int32_t* status_out, void* stream);

/* Cross-match of two source catalogues: which source of
 * catalogue 1 is which source of catalogue 2, by position.  This is what the
 * reference's four published tables results/..._MATCHED.csv hold (catalogue 1
 * the restored, catalogue 2 the original catalogue, max_sep = 1.1 pixels), and
 * what the per-star lines of application_sgp_subdivisions.py:131-139 need.
 *  M1 row r of image b takes part iff r < min(n[b], cap), its valid entry is
 *     > 0 (when valid is given) and its x and y are finite.  A non-finite
 *     coordinate on a row that passes the other two tests sets
 *     BSGP_MATCH_NONFINITE; n[b] > cap sets BSGP_MATCH_OVER_CAP and the rows
 *     beyond cap are ignored.
 *  M2 dx = x1[i] - x2[j], dy = y1[i] - y2[j], d2 = dx * dx + dy * dy, sep =
 *     sqrt(d2): float64, one rounding per operation, no fused multiply-add.
 *     (i, j) is a candidate iff sep <= max_sep (inclusive); an infinite d2 is
 *     never one.  Both catalogues' scans evaluate this expression.  (The
 *     kernels compare d2 with the largest float64 whose square root is <=
 *     max_sep, found on the host: sqrt is monotone, so the candidates are the
 *     same.)
 *  M3 candidates are strictly ordered by (d2, i, j), lexicographic.
 *  M4 the result is the greedy symmetric best match: the candidates are walked
 *     in M3's order and a pair is accepted iff neither row is taken.  The
 *     kernels compute it in rounds: every untaken row of either catalogue picks
 *     its best untaken candidate by M3 (from catalogue 2's side the key is
 *     (d2, i)), mutual picks are accepted, and a round that accepts nothing
 *     ends the loop.  A round accepts at least the smallest remaining
 *     candidate, so there are at most min(n1, n2) accepting rounds.
 *  M5 match1 [B][cap1] = j or -1, match2 [B][cap2] = i or -1, sep1 [B][cap1] =
 *     sep or NaN, npairs [B], status [B] (BSGP_MATCH_* bits).  Rows that take
 *     no part, and rows from n[b] to cap, get -1 / NaN.
 *  M6 a batch gives every image what it gets alone; the results depend neither
 *     on the launch shape nor on the path.  B == 0 is a no-op that follows no
 *     pointer.  Asynchronous on stream.
 * Element (b, r) of a column is ptr[(b * cap + r) * stride]: the catalogue
 * bsgp_segment_catalog writes is matched in place with x = f64_cols + 3, y =
 * f64_cols + 4, stride 8 and valid = int_cols, vstride 5 (area 0 marks the rows
 * of absent labels, whose zero coordinates are no points); plain arrays have
 * stride 1 and valid NULL.  n1 / n2: device int32 [B], or NULL for cap.
 * One workgroup serves one image pair.  path: BSGP_MATCH_AUTO, BSGP_MATCH_LDS
 * (coordinates and state in LDS: cap1 + cap2 <= BSGP_MATCH_LDS_MAX; the host
 * sees the caps, not n, so the caps decide) or BSGP_MATCH_GLOBAL (the same
 * algorithm on a stream-ordered global workspace: cap1, cap2 <=
 * BSGP_MATCH_MAX).  AUTO takes the LDS path where it serves the caps.
 * BSGP_ERR_UNSUPPORTED: a cap over BSGP_MATCH_MAX, or caps the chosen path does
 * not serve.  BSGP_ERR_ARG: max_sep negative or not finite, a cap < 1, B < 0,
 * a stride < 1, an unknown path, a NULL array other than valid1 / valid2 /
 * n1 / n2. */
#define BSGP_MATCH_LDS_MAX 4096
#define BSGP_MATCH_MAX 16384
#define BSGP_MATCH_AUTO 0
#define BSGP_MATCH_LDS 1
#define BSGP_MATCH_GLOBAL 2
#define BSGP_MATCH_NONFINITE 1
#define BSGP_MATCH_OVER_CAP 2
int bsgp_match_catalogs(const double* x1, const double* y1, int32_t stride1, const int32_t* valid1,
                        int32_t vstride1, int32_t cap1, const int32_t* n1, const double* x2,
                        const double* y2, int32_t stride2, const int32_t* valid2, int32_t vstride2,
                        int32_t cap2, const int32_t* n2, int32_t B, double max_sep, int32_t path,
                        int32_t* match1_out, int32_t* match2_out, double* sep1_out,
                        int32_t* npairs_out, int32_t* status_out, void* stream);

/* Star-stamp metrics: what application_sgp_star_stamps.py:117-142
 * computes for the observed and the restored stamp.  All three are
 * asynchronous; every image, profile and pair is processed on its own and gets
 * the bits it gets alone.
 *
 * bsgp_radial_profile: utils.radial_profile (restoration/utils.py:81-92).
 * r = (int)sqrt((i - c0)^2 + (j - c1)^2) with i the row and j the column:
 * centers [B][2] (device float64) holds (c0, c1), and c0 is measured along the
 * rows.  The reference passes (xcentroid, ycentroid) there; the quirk is kept.
 * prof [B][rcap] = sum of the pixels of bin k, added in raster order, over
 * their count (bit-equal to numpy.bincount's quotient; an empty bin is NaN),
 * NaN from len[b] = largest r + 1 on.  rcap must be at least every image's
 * length (the caller computes it from the shape and the centres, which must be
 * finite); bins from rcap on are dropped.  data: float32 or float64 (dtype),
 * widened first.  H * W <= 16384 and rcap <= 256, else BSGP_ERR_UNSUPPORTED. */
int bsgp_radial_profile(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                        const double* centers, int32_t rcap, double* prof, int32_t* len,
                        void* stream);
/* utils.fit_radprof (utils.py:180-202): a * exp(-0.5 (x - m)^2 / s^2) fitted
 * to (x = 0 .. len[b]-1, prof[b]) from a = 0.8 max(prof), m = 0, s = fwhm[b] /
 * (2 sqrt(2 ln 2)) by MINPACK's lmder as scipy.optimize.leastsq calls it for
 * astropy's LevMarLSQFitter: analytic Jacobian, ftol 1.49012e-8, xtol 1e-7,
 * gtol 0, maxfev 100, factor 100, mode 1; s clipped below at float32's tiny in
 * the residuals and the result, not in the Jacobian.  prof, fitted: [B][rcap]
 * (fitted: the model at x, NaN from len[b] on); len, fwhm: [B]; params [B][3]
 * = a, m, s; perr [B][3] = sqrt(|diag(cov_x sum(fvec^2) / (len - 3))|), NaN
 * where leastsq gives no cov_x (singular R, exit code not 1..4) or len <= 3;
 * info [B][2] = ier (MINPACK's info; 5 = maxfev), nfev.  len < 3, len > rcap or
 * a non-finite value inside the length: ier 0, nfev 0 and NaN everywhere.
 * rcap <= 256, else BSGP_ERR_UNSUPPORTED. */
int bsgp_fit_gauss1d(const double* prof, const int32_t* len, int32_t B, int32_t rcap,
                     const double* fwhm, double* fitted, double* params, double* perr,
                     int32_t* info, void* stream);
/* utils.wasserstein_distance_norm (utils.py:276-291), i.e.
 * scipy.stats.wasserstein_distance(u[b][:ulen[b]], v[b][:vlen[b]]) without
 * weights: the sum over the merged sorted values t of |#{u <= t} / n -
 * #{v <= t} / m| dt, in ascending order.  u, v: [B][rcap] device float64;
 * ulen, vlen: device int32 [B] (NULL: rcap); out [B].  A non-finite value
 * inside a length, or a length outside 1..rcap, gives NaN.  rcap <= 256, else
 * BSGP_ERR_UNSUPPORTED. */
int bsgp_wasserstein1(const double* u, const int32_t* ulen, const double* v, const int32_t* vlen,
                      int32_t B, int32_t rcap, double* out, void* stream);

/* Star-stamp cutouts and selection: the two ends of
 * application_sgp_star_stamps.py's loop around the solver and the metrics.
 * Both are asynchronous; n == 0 is a no-op that follows no pointer.
 *
 * bsgp_extract_stamps: Cutout2D(img, (x, y), size=(sh, sw)) in its default
 * mode 'trim' (application_sgp_star_stamps.py:58) for n positions xy [n][2]
 * (device float64; x the column, y the row).  The box is astropy 4.3.1's
 * overlap_slices: per axis imin = (int)ceil(pos - size / 2.0) in float64 and
 * imax = imin + size (imin is kept inside +-2^30; such a box overlaps no
 * image).  img: device [H][W], float32 or float64 (dtype = BSGP_DTYPE_*); out
 * [n][sh][sw] keeps that type and the values bit for bit.  box_out: int32
 * [n][4] = the untrimmed x0, y0, x1, y1 (exclusive ends).  status_out: int32
 * [n], 0 for a stamp that lies inside the image (touching the border
 * included), else one of
 *   BSGP_STAMP_PARTIAL       the box leaves the image: the pixels outside are 0
 *                            (the reference drops the stamp: its trimmed
 *                            cutout's shape is not (31, 31), :60-61)
 *   BSGP_STAMP_NO_OVERLAP    the box misses the image (astropy raises
 *                            NoOverlapError): the stamp is all 0
 *   BSGP_STAMP_BAD_POSITION  a coordinate is not finite (astropy raises
 *                            ValueError): the stamp and the box are all 0
 * BSGP_ERR_ARG: a NULL array, an unknown dtype, H, W, sh or sw < 1, n < 0;
 * BSGP_ERR_UNSUPPORTED: sh * sw > 2^24. */
#define BSGP_STAMP_PARTIAL 1
#define BSGP_STAMP_NO_OVERLAP 2
#define BSGP_STAMP_BAD_POSITION 4
int bsgp_extract_stamps(const void* img, int32_t dtype, int32_t H, int32_t W, const double* xy,
                        int32_t n, int32_t sh, int32_t sw, void* out, int32_t* box_out,
                        int32_t* status_out, void* stream);
/* bsgp_stamp_select: the choice among the K restorations of each of n stars and
 * the star's result row (application_sgp_star_stamps.py:92-98 and 125-139).
 * Image i = s * K + k is candidate k of star s.  res_nlabels [n * K]: the
 * detections of restored image i; res_cols + i * res_stride: the f64_cols row
 * of its label 1 (the reference reads element [0] of every column), as
 * bsgp_segment_catalog writes it; obs_cols + s * obs_stride: that row of the
 * observed stamp; iters [n * K]: the solver's iterations.  Strides count
 * float64 values and are at least 8.
 *   scores_out [n][K] = 1 - flux_r / flux_o, or +inf where res_nlabels <= 0
 *   best_out [n]      the reference's running minimum from +inf with a strict
 *                     comparison: the first of equal scores wins, NaN never
 *                     does; -1 when no score is below +inf (status
 *                     BSGP_STAMP_NO_CANDIDATE).  K == 1 is the sgp(...) branch
 *                     (:107-112): no search, best = 0, and a restoration
 *                     without a detection sets BSGP_STAMP_RESTORED_NO_SOURCE
 *   rows_out [n][BSGP_STAMP_ROW_COLS] = orig_flux, restored_flux,
 *                     flux_fractional_difference, fwhm_ratio, ellipticity_ratio,
 *                     then (xcentroid, ycentroid, fwhm) of the observed stamp and
 *                     of the winner; with a status bit the winner's entries are
 *                     NaN
 *   num_iters_out [n] iters of the winner, or -1
 *   status_out [n]    0 or one of the two bits
 * fwhm and ellipticity come from covar_sigx2 / sigxy / sigy2 by the formulas of
 * photutils' documentation, one rounding per operation and no fused
 * multiply-add.  The other BSGP_STAMP_* bits belong to the driver's selection
 * (no, several sources; a non-positive flux) and are set on the host.
 * BSGP_ERR_ARG: a NULL array, n < 0, K < 1, a stride < 8. */
#define BSGP_STAMP_NO_SOURCE 8
#define BSGP_STAMP_MULTI_SOURCE 16
#define BSGP_STAMP_BAD_FLUX 32
#define BSGP_STAMP_NO_CANDIDATE 64
#define BSGP_STAMP_RESTORED_NO_SOURCE 128
#define BSGP_STAMP_ROW_COLS 11
int bsgp_stamp_select(const int32_t* res_nlabels, const double* res_cols, int32_t res_stride,
                      const double* obs_cols, int32_t obs_stride, const int32_t* iters, int32_t n,
                      int32_t K, double* scores_out, int32_t* best_out, double* rows_out,
                      int32_t* num_iters_out, int32_t* status_out, void* stream);

/* Validation of detected sources: the reference's
 * utils.validation_source(image, coord, bkgmap, rmsmap, size)
 * (restoration/utils.py:313-329) for up to cap sources in each of B images, in
 * one launch.  Asynchronous; B == 0 or cap == 0 is a no-op that follows no
 * pointer.
 *   image   device [B][H][W], float32 or float64 (dtype = BSGP_DTYPE_*), NOT
 *           background-subtracted
 *   bkgmap, rmsmap   device float64 [H][W] shared by all images
 *           (maps_per_image == 0) or [B][H][W] (maps_per_image != 0)
 *   xy      device float64: (x, y) = (column, row) of source r of image b at
 *           xy + (b * cap + r) * xy_stride, xy_stride >= 2 (2: a packed
 *           [B][cap][2]; 8 with xy = f64_cols + 3: the centroid columns of
 *           bsgp_segment_catalog, read in place)
 *   n       device int32 [B]: sources of image b (rows beyond min(n, cap) are
 *           not read), or NULL: cap
 * Per source the window is the box of Cutout2D(., (x, y), (sh, sw),
 * mode='partial', fill_value=0.0): per axis it starts at (int)ceil(pos -
 * size / 2.0) (astropy 4.3.1, as bsgp_extract_stamps) and has size cells;
 * cells outside the frame hold 0.0 and take part in every statistic.  With
 * the N = sh * sw values of each window:
 *   stats_out [B][cap][3] = source_pixs, bkg, rms
 *     source_pixs  the mean of the min(3, N) largest image values, summed in
 *                  ascending order and divided in the image's own type (each
 *                  operation rounded to float32 for a float32 image), as
 *                  np.sort(c.flatten())[-3:].mean(); then widened
 *     bkg          np.median of the bkgmap values: the middle one, or (a + b) / 2
 *                  of the two middle ones
 *     rms          numpy's pairwise sum of the rmsmap values in raster order,
 *                  divided by N
 *   valid_out [B][cap]  = source_pixs > bkg + nsigma * rms (float64, strict;
 *                  the reference's nsigma is 3); 0 when a term is NaN
 *   status_out [B][cap] = 0 or BSGP_STAMP_PARTIAL (informational: the box
 *                  leaves the frame), BSGP_STAMP_NO_OVERLAP, BSGP_STAMP_BAD_POSITION
 *                  (astropy raises for both: valid = 0 and the three
 *                  statistics are NaN)
 * A NaN in a window makes that window's statistic NaN; +-inf follow IEEE.
 * Rows beyond an image's count keep valid 0, status 0 and NaN statistics.
 * BSGP_ERR_ARG: a NULL array, an unknown dtype, B, cap < 0, H, W, sh or sw < 1,
 * xy_stride < 2, a NaN nsigma; BSGP_ERR_UNSUPPORTED: sh * sw > BSGP_VALIDATE_MAX
 * (the window is held in 128 KiB of LDS), H * W >= 2^31, B > 65535. */
#define BSGP_VALIDATE_MAX 16384
int bsgp_validate_sources(const void* image, int32_t dtype, const double* bkgmap,
                          const double* rmsmap, int32_t B, int32_t H, int32_t W,
                          int32_t maps_per_image, const double* xy, int32_t xy_stride,
                          const int32_t* n, int32_t cap, int32_t sh, int32_t sw, double nsigma,
                          double* stats_out, int32_t* valid_out, int32_t* status_out,
                          void* stream);

/* ---- fitting the DIAPL PSF model ------------------
 * What the reference leaves to DIAPL's getpsf, an external C program driven by
 * psf/psf_estimation.bash with the parameters of psf/psf_steps_and_params.MD:
 * the coefficient file psf_calculate.PSF evaluates.  With the shape parameters
 * fixed (cos, sin, ax, ay, sigma_inc: getpsf.par's, as DIAPL fixes them for
 * this step) the model is linear in its coefficients, and the fit is one
 * weighted least-squares problem per frame with
 * P = nterm * ncomp unknowns, ncomp = ngauss (ldeg+1)(ldeg+2)/2,
 * nterm = (sdeg+1)(sdeg+2)/2 (36 for getpsf.par's 2 Gaussians, local degree 2,
 * spatial degree 1).  Two calls: the moments are the only pass over pixels;
 * the solve can be repeated on them with other weights or another clipping.
 * Both are asynchronous; B == 0 or cap == 0 is a no-op that follows no pointer.
 * Shape parameters are not fitted, stars are neither recentred nor chosen,
 * there are no per-pixel weights and no neighbour subtraction. */
#define BSGP_PSFFIT_MAX_COEF 108   /* P (3 Gaussians x 6 local x 6 spatial terms) */
#define BSGP_PSFFIT_MAX_STARS 4096 /* stars of one frame */
/* per star */
#define BSGP_PSFFIT_PARTIAL 1       /* the box leaves the frame: used, with the pixels inside */
#define BSGP_PSFFIT_BAD_POSITION 2  /* x or y not finite */
#define BSGP_PSFFIT_NO_OVERLAP 4    /* the box misses the frame */
#define BSGP_PSFFIT_FEW_PIXELS 8    /* fewer than ncomp fit pixels */
#define BSGP_PSFFIT_BAD_FLUX 16     /* flux not finite or <= 0 */
#define BSGP_PSFFIT_BAD_WEIGHT 32   /* weight not finite or <= 0 (the solve) */
#define BSGP_PSFFIT_CLIPPED 64      /* dropped by a clipping round (the solve) */
#define BSGP_PSFFIT_EXCLUDED (2 | 4 | 8 | 16 | 32)
/* per frame */
#define BSGP_PSFFIT_SINGULAR 128    /* a scaled pivot not finite or <= P * 2^-52 */

/* Per-star moments of the fit.
 *   image   device [B][H][W], float32 or float64 (dtype = BSGP_DTYPE_*)
 *   xy      device float64 [B][cap][2]: (x, y) = (column, row), 0-based
 *   n       device int32 [B]: stars of frame b, or NULL: cap
 *   model   host: hw, ngauss, ldeg, sdeg, cos, sin, ax, ay, sigma_inc, x_orig,
 *           y_orig (coeffs and ncoef are not read)
 *   fitrad  a pixel of the (2hw+1)^2 box about (floor(x + 0.5), floor(y + 0.5))
 *           that lies in the frame counts when x'^2 + y'^2 <= fitrad^2 for its
 *           offsets x' = c - x, y' = r - y, its value minus the sky is finite,
 *           its mask byte is 0 and (has_sat) its value is < sat_level
 *   flux    device [B][cap], or NULL: the sum of (I - sky) over the fit pixels
 *           in row-major order
 *   sky     sky_mode 0: none (NULL); 1: device [B][cap], one value per star;
 *           2: device float64 [B][H][W] maps
 *   mask    device bytes [B][H][W], nonzero = skipped, or NULL
 * With z = (phi_0 .. phi_{ncomp-1}, v), phi_k the terms exp(rr_g) x'^m y'^n of
 * calc_psf_pix (psf_calculate.py:52-87) in its loop order and
 * v = (I - sky) / flux, every product rounded and added in pixel order:
 *   G_out    [B][cap][ncomp (ncomp+1) / 2]  sum phi_i phi_j, packed upper
 *            triangle, rows in order
 *   h_out    [B][cap][ncomp]   sum phi_i v
 *   vv_out   [B][cap]          sum v v
 *   npix_out [B][cap], flux_out [B][cap] (the flux used), status_out [B][cap]
 * An excluded star (BSGP_PSFFIT_EXCLUDED) has zero moments.  Rows beyond a
 * frame's count are zero.
 * BSGP_ERR_ARG: a NULL array, an unknown dtype or sky_mode, B, cap < 0, H,
 * W < 1, hw outside 0..255, a degree < 0, ngauss < 1, fitrad not > 0;
 * BSGP_ERR_UNSUPPORTED: P > BSGP_PSFFIT_MAX_COEF, cap > BSGP_PSFFIT_MAX_STARS,
 * H * W >= 2^31, B > 65535. */
int bsgp_psf_fit_moments(const void* image, int32_t dtype, int32_t B, int32_t H, int32_t W,
                         const double* xy, const int32_t* n, int32_t cap,
                         const bsgp_psf_model* model, double fitrad, const double* flux,
                         const double* sky, int32_t sky_mode, const uint8_t* mask, int32_t has_sat,
                         double sat_level, double* G_out, double* h_out, double* vv_out,
                         int32_t* npix_out, double* flux_out, int32_t* status_out, void* stream);

/* The coefficients from the moments (getpsf's NSIG_CLIP / NITER rounds
 * included), one workgroup per frame, no host round trip between rounds.
 *   xy, n, model, G, h, vv, npix, mstatus   as given to / written by
 *           bsgp_psf_fit_moments
 *   weights device [B][cap], or NULL: 1
 * N = sum w (S S^T) (x) G and b = sum w S (x) h over the active stars in index
 * order, S the spatial terms (x - x_orig)^m (y - y_orig)^n of init_psf
 * (psf_calculate.py:140-165); N is scaled by its diagonal, Cholesky-factored and
 * solved.  Per star rss = max(0, vv - 2 c.h + c.G c) with c the local
 * coefficients at the star, rms = sqrt(rss / npix).  A clipping round drops
 * the active stars with rms > median + nsig * 1.4826 * MAD (of the active
 * stars' rms) and rss > 4096 * 2^-52 * vv, if it drops any and at least
 * max(nterm, min_stars) remain; the fit is then repeated, at most niter times.
 *   coef_out   [B][P], term-major as a coefficient file; NaN when singular
 *   used_out   [B][cap] 0 / 1, status_out [B][cap] (mstatus plus the solve's bits)
 *   rms_out    [B][cap] of the last fit a star took part in; NaN for a star
 *              never active and for every star of a singular frame
 *   frame_out  [B][3]: 0 or BSGP_PSFFIT_SINGULAR, rounds applied, stars used
 * BSGP_ERR_ARG / BSGP_ERR_UNSUPPORTED as bsgp_psf_fit_moments; niter < 0,
 * min_stars < 0 or a NaN nsig is BSGP_ERR_ARG. */
int bsgp_psf_fit_solve(int32_t B, int32_t cap, const int32_t* n, const double* xy,
                       const bsgp_psf_model* model, const double* G, const double* h,
                       const double* vv, const int32_t* npix, const int32_t* mstatus,
                       const double* weights, int32_t niter, double nsig, int32_t min_stars,
                       double* coef_out, int32_t* used_out, int32_t* status_out, double* rms_out,
                       int32_t* frame_out, void* stream);

/* ---- finding and measuring a frame's stars --------
 * What the reference leaves to DIAPL's sfind and fwhmm (psf/psf_estimation.bash,
 * psf/psf_steps_and_params.MD) and the star choice of getpsf: from a frame to
 * the rows of a .coo file (x y approx_flux local_bkg_level num_saturated) and to
 * the PSF stars bsgp_psf_fit_moments takes.  DIAPL's source is not part of the
 * reference, so the rule is this library's own, modelled on the published
 * parameter files and restated in numpy in tests/starfind_ref.py.  Float64
 * arithmetic on float32 or float64 frames, every product and sum rounded, no
 * floating-point atomics: a batch gives each frame the bits it gets alone.
 * All four calls are asynchronous.
 *
 * The template (F1) is built by the caller and shared by all calls: for
 * rap = aprad * fwhm and R = floor(rap) <= BSGP_STARFIND_MAX_R the support is
 * the offsets |dy| <= R, |dx| <= halfw[dy + R] (the dx with dx^2 + dy^2 <=
 * rap^2) in row-major order, n of them; tmpl[n] on the device holds
 * t = g - mean(g), g = exp(-(dx^2 + dy^2) / (2 sigma^2)), and tt = sum t^2.
 *   halfw   HOST int32 [2R + 1], each in 0..R */
#define BSGP_STARFIND_MAX_R 15
#define BSGP_STARFIND_MAX 16384 /* stars of one frame */
/* per star (icols' status) */
#define BSGP_STARFIND_BAD_FLUX 1     /* aperture flux not finite or <= 0 */
#define BSGP_STARFIND_OFF_CENTRE 2   /* brightest pixel farther than dxy from (x, y) */
#define BSGP_STARFIND_FEW_SKY 4      /* fewer than min_sky annulus values */
#define BSGP_STARFIND_SKY_OVER_CAP 8 /* more than BSGP_LOCALBKG_MAX annulus values */
#define BSGP_STARFIND_REJECTED (1 | 2 | 4 | 8)
/* per frame (bsgp_star_peaks' status_out) */
#define BSGP_STARFIND_OVER_CAP 16 /* more candidates than cap: the first cap are kept */
#define BSGP_STARFIND_BKG_MODE 0
#define BSGP_STARFIND_BKG_MEDIAN 1
#define BSGP_STARFIND_BKG_MEAN 2

/* F2, F3: the maps.  Pixel p is valid when its whole support lies in the
 * frame and every support pixel is finite and unmasked; otherwise both maps
 * hold NaN at p.  Over the support in its order s1 = sum I, s2 = sum I I,
 * st = sum t I; var = s2 - s1 s1 / n; amp = st / tt;
 * corr = st / sqrt(tt var) if var > 0, else 0.
 *   image   device [B][H][W], float32 or float64 (dtype = BSGP_DTYPE_*)
 *   mask    device bytes [B][H][W], nonzero = masked, or NULL
 *   corr_out, amp_out   device float64 [B][H][W]
 * BSGP_ERR_ARG: a NULL array, an unknown dtype, R < 0, a halfw outside 0..R,
 * tt not > 0; BSGP_ERR_UNSUPPORTED: R > BSGP_STARFIND_MAX_R, H * W >= 2^31,
 * B > 65535. */
int bsgp_star_maps(const void* image, int32_t dtype, int32_t B, int32_t H, int32_t W,
                   const uint8_t* mask, const double* tmpl, const int32_t* halfw, int32_t R,
                   double tt, double* corr_out, double* amp_out, void* stream);

/* F4, F5: the candidates.  p is one when it is valid (amp is not NaN),
 * corr >= c_min, st >= (thresh * noise(p)) * sqrt(tt) (st added again from the
 * frame exactly as the maps added it) and amp(p) is the maximum of the
 * (2 peak_hw + 1)^2 window over valid pixels, strictly above those earlier in
 * raster order and >= those later.  Numbered in raster order per frame.
 *   noise      device float64 [B] (noise_is_map == 0) or [B][H][W]
 *   peaks_out  device int32 [B][cap][2]: column, row of candidate r of frame b
 *   n_out      device int32 [B]: min(candidates, cap)
 *   status_out device int32 [B]: 0 or BSGP_STARFIND_OVER_CAP
 * BSGP_ERR_ARG as bsgp_star_maps, and peak_hw outside 0..3, cap < 1, a NaN
 * c_min or thresh; BSGP_ERR_UNSUPPORTED: cap > BSGP_STARFIND_MAX. */
int bsgp_star_peaks(const void* image, int32_t dtype, int32_t B, int32_t H, int32_t W,
                    const double* corr, const double* amp, const double* tmpl,
                    const int32_t* halfw, int32_t R, double tt, const double* noise,
                    int32_t noise_is_map, double c_min, double thresh, int32_t peak_hw,
                    int32_t cap, int32_t* peaks_out, int32_t* n_out, int32_t* status_out,
                    void* stream);

/* F6 to F8: one workgroup per candidate.
 * Sky: the pixels with anrad1^2 <= dx^2 + dy^2 <= anrad2^2 about the peak
 * pixel (ic, ir) that lie in the frame, are finite, unmasked and (has_sat)
 * < sat_level, sorted and sigma-clipped (median -+ sigma * std, at most
 * maxiters rounds; the local background's L4) and reduced by bkg_alg: MODE is
 * the local background's L5 (mean if std == 0, 2.5 median - 1.5 mean if
 * |mean - median| / std < 0.3, else median), MEDIAN and MEAN the clipped ones.
 * Fewer than min_sky values: bkg NaN and FEW_SKY; more than BSGP_LOCALBKG_MAX:
 * bkg NaN and SKY_OVER_CAP.
 * Aperture: the template's support about (ic, ir) with J = I - bkg; each
 * support row left to right, then the row sums top to bottom:
 * F = sum J, Sx = sum dx J, Sy = sum dy J, Sxx = sum (dx dx) J, Syy, Sxy;
 * x = ic + Sx / F, y = ir + Sy / F,
 * fwhm = 2 sqrt(2 ln 2) sqrt(((Sxx / F - (Sx / F)^2) + (Syy / F - (Sy / F)^2)) / 2),
 * NaN unless the argument is > 0; peak = max I - bkg, the brightest pixel the
 * first maximum in raster order; nsat counts support pixels >= sat_level.
 * BAD_FLUX: F not finite or <= 0; OFF_CENTRE: the brightest pixel's squared
 * distance from (x, y) exceeds dxy^2.
 *   peaks, n   as bsgp_star_peaks wrote them
 *   fcols_out  device float64 [B][cap][8]: x, y, flux, bkg, peak, corr, amp, fwhm
 *   icols_out  device int32 [B][cap][4]: ic, ir, nsat, status
 * Rows beyond a frame's count are NaN / 0.
 * BSGP_ERR_ARG: a NULL array, not 0 <= anrad1 < anrad2, an unknown bkg_alg,
 * maxiters < 0, min_sky < 1, a NaN sigma or dxy; BSGP_ERR_UNSUPPORTED:
 * anrad2 >= 1025, and as above. */
int bsgp_star_measure(const void* image, int32_t dtype, int32_t B, int32_t H, int32_t W,
                      const uint8_t* mask, const double* corr, const double* amp,
                      const int32_t* halfw, int32_t R, const int32_t* peaks, const int32_t* n,
                      int32_t cap, double anrad1, double anrad2, int32_t bkg_alg, double sigma,
                      int32_t maxiters, int32_t min_sky, int32_t has_sat, double sat_level,
                      double dxy, double* fcols_out, int32_t* icols_out, void* stream);

/* F9: the PSF stars.  A star without a BSGP_STARFIND_REJECTED bit ("kept") is
 * eligible when flux >= min_flux, nsat == 0, (has_max_peak) peak <= max_peak,
 * the (2 hw + 1)^2 box about (floor(x + 0.5), floor(y + 0.5)) lies in the
 * frame, and no other kept star t with flux_t >= rat_thresh * flux has
 * dx dx + dy dy <= iso_radius^2.  Its rank is the number of eligible stars
 * that are brighter, or equally bright with a smaller index; it is selected
 * when the rank is below npsf_max.
 *   fcols, icols   as bsgp_star_measure wrote them; n device [B] or NULL: cap
 *   eligible_out, rank_out (-1: not eligible), selected_out   device int32 [B][cap]
 * BSGP_ERR_ARG: a NULL array, B or cap < 0, H, W < 1, hw < 0, npsf_max < 0, a
 * NaN among the numbers; BSGP_ERR_UNSUPPORTED: cap > BSGP_STARFIND_MAX,
 * B > 65535.  B == 0 or cap == 0 is a no-op. */
int bsgp_star_select(const double* fcols, const int32_t* icols, const int32_t* n, int32_t B,
                     int32_t cap, int32_t H, int32_t W, int32_t hw, double min_flux,
                     int32_t has_max_peak, double max_peak, double rat_thresh,
                     double iso_radius, int32_t npsf_max, int32_t* eligible_out,
                     int32_t* rank_out, int32_t* selected_out, void* stream);

int bsgp_device_synchronize(void);
const char* bsgp_last_error(void);
/* The persistent solver's compile-time-geometry path (256 x 256 images on a
 * 270 x 270 grid, linear mode, float64 storage, one workgroup per image: the
 * same results bit for bit, fewer instructions).  bsgp_plan_set_static_geo
 * chooses for the NEXT solve or resume on the plan only: 1 take it where the
 * plan matches, 0 never, -1 the default (environment BSGP_STATIC_GEO, else 1).
 * bsgp_plan_static_geo reports whether the plan's last solve took it. */
int bsgp_plan_set_static_geo(bsgp_plan plan, int32_t mode);
int bsgp_plan_static_geo(bsgp_plan plan, int32_t* used);

int32_t bsgp_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BSGP_H_ */
