// bsgp_apps.hpp — the application stages' argument blocks, limits and launch
// declarations: what their kernel units (bsgp_tiles, bsgp_coadd, bsgp_psf,
// bsgp_background, bsgp_segment, bsgp_convolve, bsgp_localbkg, bsgp_match,
// bsgp_deblend, bsgp_stamps, bsgp_starstamps, bsgp_validate, bsgp_psffit, bsgp_starfind .hip) share
// with the C-ABI host layer (bsgp_apps.hip).  Nothing of the solver.  Not part of the public interface.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/bsgp.h"
#include "bsgp_psffit.hpp"  // PsfShape

namespace bsgp {

// ---- tiles, FITS pixels, PSF stamps (bsgp_tiles.hip, bsgp_psf.hip) ----------
hipError_t launch_extract_tiles(const double* img, int W, const int* boxes, int n, int th, int tw,
                                double* out, hipStream_t s);
hipError_t launch_coadd_tiles(const double* tiles, int n, int th, int tw, const int* boxes, int H,
                              int W, double* mean, double* footprint, hipStream_t s);
hipError_t launch_fits_to_f64(const void* raw, int64_t n, int bitpix, double bscale, double bzero,
                              double* out, hipStream_t s);
struct PsfModel;  // bsgp_psf.hpp
hipError_t launch_psf_stamps(const PsfModel& m, const double* xy, int n, int spatial,
                             int normalize, double* out, hipStream_t s);
// ---- background-matched co-add (bsgp_coadd.hip) ------
// relative residual |b - L c| / |b| at which the conjugate gradients stop (the recurrence's
// residual; the corrections then sit within cond(L) * this of the solution: 1e-13 * 30 on
// the tile grids of the application, under the 1e-10 at which reproject's solver stops)
constexpr double kCoaddRtol = 1e-13;
constexpr int kCoaddLdsMax = 160 * 1024 - 256;  // dynamic LDS of the matched co-add
struct CoaddOffsetArgs {
  const double* tiles;  // [n][th][tw]
  const int* boxes;     // [n][4] xyxy
  const int* pairs;     // [npairs][2], i < j
  int n, th, tw, npairs;
  double* offsets;  // [npairs]
  int* status;      // [n], BSGP_COADD_* bits
};
struct CoaddSolveArgs {
  int n, ncomp, bref;  // bref < 0: no background reference
  const int *row_ptr, *nbr, *nbr_pair, *nbr_sign;  // adjacency lists (CSR) over the pairs
  const int* component;                            // [n], 0 .. ncomp - 1
  const double* offsets;                           // [npairs], NaN: the pair is dropped
  double* c;       // [n] out
  int* status;     // [n], bits are added
  double* ws;      // [2 n]: residual, L p
  double* info;    // [2] out (iterations, relative residual), or nullptr
};
hipError_t launch_pair_offsets(const CoaddOffsetArgs& a, hipStream_t s);
hipError_t launch_solve_corrections(const CoaddSolveArgs& a, hipStream_t s);
hipError_t launch_coadd_tiles_matched(const double* tiles, int n, int th, int tw, const int* boxes,
                                      const double* corr, int H, int W, double* mean,
                                      double* footprint, hipStream_t s);
// ---- sky background (bsgp_background.hip) ----------------------
constexpr int kBkgMaxBox = 4096;    // pixels of one box: its sorted copy is 32 KiB of LDS
constexpr int kBkgMaxCells = 4096;  // cells of one image's mesh (k_bkg_mesh keeps two copies in LDS)
constexpr int kBkgMaxFilter = 7;    // median filter window, per axis
constexpr int kBkgZoomLine = 520;   // k_bkg_zoom's folded coefficient line (512 pixels / bw + 4)
// Arguments of the three background kernels (by value: scalar loads).
struct BkgArgs {
  const void* data;           // [B][H][W] float32 or float64
  const unsigned char* mask;  // [B][H][W] bytes, nonzero = masked, or nullptr
  int B, H, W, bh, bw, fh, fw, ny, nx, maxiters, clip;
  double sigma;
  double excl_count;  // a box with more invalid pixels than this is excluded
  // per image: raw median / std meshes, filtered meshes, spline coefficients
  // (2 x ny*nx each), then {min, max} of both filtered meshes and their medians
  double* ws;
  size_t ws_stride;  // doubles per image: 6 * ny*nx + 8
  int* wsi;          // per image: kept cells, then excluded / survivors / iterations [ny*nx] each
  double *bkg, *rms, *mesh, *rms_mesh, *medians;  // outputs, any may be nullptr
  int* status;                                    // output copy of wsi, or nullptr
};
hipError_t launch_bkg_boxstats(const BkgArgs& a, int f32, hipStream_t s);
hipError_t launch_bkg_mesh(const BkgArgs& a, hipStream_t s);
hipError_t launch_bkg_zoom(const BkgArgs& a, hipStream_t s);
// ---- source detection (bsgp_segment.hip) ----------------------
constexpr int kSegMaxKernel = 7;  // convolution kernel, per axis (odd)
constexpr int kSegChunk = 2048;   // pixels one workgroup numbers in the compaction
struct SegConvArgs {
  const void* data;      // [B][H][W] float32 or float64
  const double* kernel;  // [kh][kw] on the device
  double* out;           // [B][H][W]
  int B, H, W, kh, kw;
};
struct SegArgs {
  const void* data;           // [B][H][W] float32 or float64
  const double* thr_map;      // [B][H][W], or nullptr: thr
  const unsigned char* mask;  // [B][H][W] bytes, nonzero = never detected, or nullptr
  double thr;
  int B, H, W, npixels, conn, nblk;  // nblk: chunks of kSegChunk pixels per image
  int* lab;                          // workspace [B][H*W]: union-find parents (-1: background)
  int* area;                         // workspace [B][H*W]: a root's area, then its final label
  int* blk;                          // workspace [B][nblk]: kept roots per chunk, then their scan
  int* labels_out;                   // [B][H][W]
  int* nlabels_out;                  // [B]
};
struct SegCatArgs {
  const double* data;  // [B][H][W]
  const double* conv;  // [B][H][W], or nullptr: data
  const int* labels;   // [B][H][W]
  const int* nlabels;  // [B], or nullptr: cap
  int B, H, W, cap;
  int* icols;     // [B][cap][5]: area, xmin, xmax, ymin, ymax
  double* fcols;  // [B][cap][8]: flux, min, max, xc, yc, sigx2, sigxy, sigy2
  int* status;    // [B]: bit 0 nlabels > cap, bit 1 a label outside 1..min(cap, nlabels)
};
hipError_t launch_seg_convolve(const SegConvArgs& a, int f32, hipStream_t s);
hipError_t launch_seg_detect(const SegArgs& a, int f32, hipStream_t s);
hipError_t launch_seg_catalog(const SegCatArgs& a, hipStream_t s);
// ---- PSF-sized convolution (bsgp_convolve.hip) ----------------
constexpr int kConvMaxKernel = BSGP_CONV_MAX_KERNEL;  // per axis (odd)
struct ConvArgs {
  const void* data;           // [B][H][W] float32 or float64
  const double* kernel;       // [kh][kw], or [B][kh][kw] at kernel_stride = kh * kw
  const double* kernel_sum;   // [1], or [B] with per-image kernels
  const unsigned char* mask;  // [B][H][W] bytes, nonzero = masked, or nullptr
  double fill_value;
  double* out;  // [B][H][W]
  int* status;  // [B]: BSGP_CONV_HAD_NAN | BSGP_CONV_NAN_LEFT
  int B, H, W, kh, kw, kernel_stride, flags;
  int ntx;  // tiles per tile row (the launch fills it in)
};
int conv_rows_per_thread(int H, int kh, int kw);
int64_t conv_tiles(int H, int W, int kh, int kw);  // workgroups per image
hipError_t launch_convolve(const ConvArgs& a, int f32, hipStream_t s);
// ---- local background (bsgp_localbkg.hip) ------------
constexpr int kLocalBkgMax = BSGP_LOCALBKG_MAX;  // values of one annulus: 64 KiB of LDS
struct LocalBkgArgs {
  const void* data;    // [B][H][W] float32 or float64
  const int* labels;   // [B][H][W]
  const int* nlabels;  // [B], or nullptr: cap
  const int* icols;    // [B][cap][5] as bsgp_segment_catalog writes them
  double* fcols;       // [B][cap][8]: flux, min, max corrected in place when apply
  int B, H, W, cap, maxiters, min_pixels, apply;
  double width, sigma;
  double* lb;   // [B][cap] (zeroed first)
  int* npix;    // [B][cap][2]: values gathered, survivors (zeroed first)
  int* status;  // [B]: BSGP_LOCALBKG_* bits (zeroed first)
};
hipError_t launch_localbkg(const LocalBkgArgs& a, int f32, hipStream_t s);
// ---- catalogue cross-match (bsgp_match.hip) ----------
constexpr int kMatchLdsMax = BSGP_MATCH_LDS_MAX;  // cap1 + cap2 of the LDS path
constexpr int kMatchMax = BSGP_MATCH_MAX;         // rows of one catalogue
// One side's columns: element (b, r) is ptr[(b * cap + r) * stride].
struct MatchCat {
  const double *x, *y;
  const int* valid;  // > 0 = the row takes part, or nullptr: every row
  const int* n;      // [B], or nullptr: cap
  int stride, vstride, cap;
};
struct MatchArgs {
  MatchCat c1, c2;
  double d2_lim;  // a candidate has d2 < d2_lim: the float64 after the largest whose sqrt <= max_sep
  int *match1, *match2;  // [B][cap1], [B][cap2]
  double* sep1;          // [B][cap1]
  int *npairs, *status;  // [B]
  // the global path's workspace, per image: (x, y) of match_rows(cap1, cap2)
  // rows, then their best and match entries
  double* ws_xy;
  int* ws_state;
};
// rows of the kernels' joint index space: catalogue 2 starts on a wave boundary
__host__ __device__ inline int match_rows(int n1, int n2) { return ((n1 + 63) & ~63) + n2; }
constexpr size_t kMatchRowBytes = 2 * sizeof(double) + 2 * sizeof(int);
// block: threads per workgroup, a multiple of 64 up to 1024
hipError_t launch_match(const MatchArgs& a, int B, bool lds, int block, hipStream_t s);
// ---- deblending (bsgp_deblend.hip) -----------------------------
constexpr int kDeblendMaxBox = BSGP_DEBLEND_MAX_BOX;  // box pixels of one parent (LDS)
struct DeblendArgs {
  const double* data;        // [B][H][W]
  const int* labels;         // [B][H][W]
  const int* nlabels;        // [B]
  const int* icols;          // [B][cap][5] as bsgp_segment_catalog writes them
  const unsigned char* sel;  // [B][cap], nonzero = deblend this label, or nullptr: all
  int B, H, W, cap, npixels, nlevels, conn, mode;
  double contrast;
  int* nchild;       // workspace [B][cap]: children of a split parent, else 0 (zeroed first)
  int* base;         // workspace [B][cap]: a parent's output label / its first child's
  int* labels_out;   // [B][H][W]: child ranks of split parents, then the final labels
  int* nlabels_out;  // [B]
  int* status;       // [B]: BSGP_DEBLEND_* bits (zeroed first)
  // k_deblend_large (large != 0): parents whose box holds more than lds_max_box
  // pixels.  Workspace per image pixel, never initialised: a parent writes its
  // own pixels' entries before it reads them.
  int lds_max_box, large;
  int* lev;      // [B][H*W]: the level's union-find parents (-1: not above the level)
  int* reg;      // [B][H*W]: the region (its root) a pixel is in, or kFree
  int* cnt;      // [B][H*W]: a root's component area
  int* kept;     // [B][H*W]: kept roots per region; then a marker's list index, then its rank
  int* mk;       // [B][H*W]: marker lists, a parent's at the sum of the image's lower areas
  int* hidx;     // [B][H*W]: heap entries beyond the LDS part, pixel indices, at the same offset
  double* hkey;  // [B][H*W]: their keys
};
constexpr int kDeblendLargeMaxArea = BSGP_DEBLEND_LARGE_MAX_AREA;
hipError_t launch_deblend(const DeblendArgs& a, hipStream_t s);
// ---- star-stamp metrics (bsgp_stamps.hip) ----------------------
constexpr int kStampMaxPixels = 16384;  // H * W of one stamp
constexpr int kStampMaxBins = 256;      // radial bins / profile length / sample length
struct StampProfArgs {
  const void* data;       // [B][H][W] float32 or float64
  const double* centers;  // [B][2]: (along rows, along columns)
  int B, H, W, rcap;
  double* prof;  // [B][rcap], NaN beyond an image's length
  int* len;      // [B]: largest bin + 1
};
struct StampFitArgs {
  const double* prof;  // [B][rcap]
  const int* len;      // [B]
  const double* fwhm;  // [B]
  int B, rcap;
  double *fitted, *params, *perr;  // [B][rcap], [B][3], [B][3]
  int* info;                       // [B][2]: ier, nfev
};
struct StampW1Args {
  const double *u, *v;     // [B][rcap]
  const int *ulen, *vlen;  // [B], or nullptr: rcap
  int B, rcap, P;          // P: power of two >= 2 rcap (the sort's size)
  double* out;             // [B]
};
hipError_t launch_stamp_radprof(const StampProfArgs& a, int f32, hipStream_t s);
hipError_t launch_stamp_fit(const StampFitArgs& a, hipStream_t s);
hipError_t launch_stamp_w1(const StampW1Args& a, hipStream_t s);
// ---- star-stamp cutouts and selection (bsgp_starstamps.hip) ----
constexpr int kStampCutMaxPixels = 1 << 24;  // sh * sw of one cutout (an int index per stamp)
constexpr int kStampBoxLimit = 1 << 30;      // |imin| of a box: imin + size stays an int
constexpr int kStampRowCols = BSGP_STAMP_ROW_COLS;
struct StampCutArgs {
  const void* img;   // [H][W] float32 or float64
  const double* xy;  // [n][2]: (x, y) = (column, row)
  int H, W, n, sh, sw;
  void* out;    // [n][sh][sw] in the image's type
  int* box;     // [n][4]: the untrimmed x0, y0, x1, y1
  int* status;  // [n]: BSGP_STAMP_PARTIAL / NO_OVERLAP / BAD_POSITION
};
struct StampSelectArgs {
  const int* res_nlabels;   // [n * K]
  const double* res_cols;   // row of label 1 of restored image i at res_cols + i * res_stride
  const double* obs_cols;   // row of label 1 of observed stamp s at obs_cols + s * obs_stride
  const int* iters;         // [n * K]
  int n, K, res_stride, obs_stride;
  double* scores;  // [n][K]
  int* best;       // [n]
  double* rows;    // [n][kStampRowCols]
  int* num_iters;  // [n]
  int* status;     // [n]: BSGP_STAMP_NO_CANDIDATE / RESTORED_NO_SOURCE
};
hipError_t launch_extract_stamps(const StampCutArgs& a, int f32, hipStream_t s);
hipError_t launch_stamp_select(const StampSelectArgs& a, hipStream_t s);
// ---- source validation (bsgp_validate.hip) -----------
constexpr int kValidateMax = BSGP_VALIDATE_MAX;  // sh * sw of one window: 128 KiB of LDS
struct ValidateArgs {
  const void* img;              // [B][H][W] float32 or float64, not background-subtracted
  const double *bkg, *rms;      // [H][W], or [B][H][W] when maps_per_image
  const double* xy;             // (x, y) of row (b, r) at xy + (b * cap + r) * xy_stride
  const int* n;                 // [B], or nullptr: cap
  int B, H, W, maps_per_image, xy_stride, cap, sh, sw;
  int P;                        // the power of two >= sh * sw (the sort's size; the launch fills it in)
  double nsigma;
  double* stats;  // [B][cap][3]: source_pixs, bkg, rms
  int* valid;     // [B][cap]
  int* status;    // [B][cap]: BSGP_STAMP_PARTIAL / NO_OVERLAP / BAD_POSITION
};
hipError_t launch_validate(ValidateArgs a, int f32, hipStream_t s);
// ---- PSF fit (bsgp_psffit.hip) -----------------------
constexpr int kPsfFitMaxCoef = BSGP_PSFFIT_MAX_COEF;    // P: the packed normal matrix is 46 KiB of LDS
constexpr int kPsfFitMaxStars = BSGP_PSFFIT_MAX_STARS;  // per frame: their rms is sorted in 32 KiB
struct PsfFitMomentArgs {
  const void* img;            // [B][H][W] float32 or float64
  const double* xy;           // [B][cap][2]: (x, y) = (column, row)
  const int* n;               // [B], or nullptr: cap
  const double* flux;         // [B][cap], or nullptr: the sum of I - sky over the fit pixels
  const double* sky;          // sky_mode 0: none; 1: [B][cap] per star; 2: [B][H][W] maps
  const unsigned char* mask;  // [B][H][W] bytes, nonzero = skipped, or nullptr
  PsfShape shape;
  int B, H, W, cap, sky_mode, has_sat;
  int chunk;  // candidates per round of the box walk (the launch fills it in)
  double fitrad2, sat_level;
  double *G, *h, *vv;  // [B][cap][ncomp (ncomp + 1) / 2], [B][cap][ncomp], [B][cap] (zeroed first)
  double* flux_out;    // [B][cap]
  int *npix, *status;  // [B][cap] (zeroed first)
};
struct PsfFitSolveArgs {
  const double* xy;       // [B][cap][2]
  const int* n;           // [B], or nullptr: cap
  const double *G, *h, *vv;
  const int *npix, *mstatus;  // as the moments wrote them
  const double* weights;      // [B][cap], or nullptr: 1
  PsfShape shape;
  int B, cap, niter, min_stars;
  int sortP;  // the power of two >= cap (the launch fills it in)
  double nsig;
  double* coef;        // [B][P]
  double* rms;         // [B][cap]
  int *used, *status;  // [B][cap]
  int* frame;          // [B][3]: status, rounds, stars used
};
int psffit_chunk(int ncomp);
hipError_t launch_psffit_moments(PsfFitMomentArgs a, int f32, hipStream_t s);
hipError_t launch_psffit_solve(PsfFitSolveArgs a, hipStream_t s);
// ---- star finding (bsgp_starfind.hip) ---------------
constexpr int kStarMaxR = BSGP_STARFIND_MAX_R;  // the tile, its halo and the template: 30 KiB of LDS
constexpr int kStarMax = BSGP_STARFIND_MAX;     // stars of one frame
constexpr int kStarChunk = 2048;                // pixels one workgroup numbers in the compaction
constexpr int kStarMaxBox = 1024;               // floor(anrad2): the annulus' box stays an int count
// F1 (by value: scalar loads): row dy of the support is |dx| <= halfw[dy + R]
struct StarTemplate {
  const double* t;  // [n] on the device, the support's row-major order
  int R, n;
  double tt, sqrt_tt;
  signed char halfw[2 * kStarMaxR + 1];
};
struct StarMapArgs {
  const void* data;           // [B][H][W] float32 or float64
  const unsigned char* mask;  // [B][H][W] bytes, nonzero = masked, or nullptr
  StarTemplate tp;
  int B, H, W;
  double *corr, *amp;  // [B][H][W]
};
struct StarPeakArgs {
  const void* data;          // [B][H][W] float32 or float64
  const double *corr, *amp;  // [B][H][W] as k_star_maps wrote them
  const double* noise;       // [B], or [B][H][W] when noise_map
  StarTemplate tp;
  int B, H, W, noise_map, peak_hw, cap, nblk;  // nblk: chunks of kStarChunk pixels per frame
  double c_min, thresh;
  unsigned char* flag;  // workspace [B][nblk][256]: the candidate bits of a lane's 8 pixels
  int* blk;             // workspace [B][nblk]: candidates per chunk, then their scan
  int* peaks;           // [B][cap][2]: ic, ir
  int *n, *status;      // [B]
};
struct StarMeasureArgs {
  const void* data;           // [B][H][W] float32 or float64
  const unsigned char* mask;  // [B][H][W] bytes, or nullptr
  const double *corr, *amp;   // [B][H][W]
  const int* peaks;           // [B][cap][2]
  const int* n;               // [B]
  int B, H, W, cap, R, box, bkg_alg, maxiters, min_sky, has_sat;  // box: floor(anrad2)
  double r1sq, r2sq, sigma, sat_level, dxy2;
  signed char halfw[2 * kStarMaxR + 1];
  double* fcols;  // [B][cap][8]: x, y, flux, bkg, peak, corr, amp, fwhm (NaN first)
  int* icols;     // [B][cap][4]: ic, ir, nsat, status (zeroed first)
};
struct StarSelectArgs {
  const double* fcols;  // [B][cap][8]
  const int* icols;     // [B][cap][4]
  const int* n;         // [B], or nullptr: cap
  int B, cap, H, W, hw, has_max_peak, npsf_max;
  double min_flux, max_peak, rat_thresh, iso2;
  int *eligible, *rank, *selected;  // [B][cap] (0, -1, 0 first)
};
int star_annulus_pixels(double r1sq, double r2sq, int box);  // of an annulus inside the frame
hipError_t launch_star_maps(const StarMapArgs& a, int f32, hipStream_t s);
hipError_t launch_star_peaks(const StarPeakArgs& a, int f32, hipStream_t s);
hipError_t launch_star_measure(const StarMeasureArgs& a, int f32, hipStream_t s);
hipError_t launch_star_select(const StarSelectArgs& a, hipStream_t s);

}  // namespace bsgp
