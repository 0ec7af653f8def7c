/* bigstitch.h — C ABI of libbigstitch, the MI355X-native replacement for the
 * math layer of BigStitcher-Spark's two hot paths.
 *
 * Drop-in boundary (see SURVEY.md §8(b) and INTEGRATION.md):
 *
 *   bs_stitch_batch  replaces the in-process call site
 *     net.preibisch.stitcher.algorithm.globalopt.TransformationTools
 *         .computeStitching(groupA, groupB, vrs, params, sd, gva, ds, service)
 *       -> Pair<Pair<AffineGet,Double>, RealInterval>
 *     called from reference SparkPairwiseStitching.java:247-255.
 *     One bs_pair_desc = one tile-pair RDD element (SparkPairwiseStitching.java:192-303).
 *
 *   bs_fuse_blocks  replaces the in-process call site
 *     net.preibisch.mvrecon.process.fusion.blk.BlkAffineFusion
 *         .initWithIntensityCoefficients(conv, imgLoader, views, regs, vds,
 *             fusionType, ..., interp=1, coeffs, bbox, type, blockSize)
 *       -> BlockSupplier<T>   (+ the materializing BlockAlgoUtils.arrayImg copy)
 *     called from reference SparkAffineFusion.java:602-615, :627.
 *     One bs_block_desc = one output-grid element of Grid.create(dims,
 *     computeBlockSize, blockSize) (SparkAffineFusion.java:459-461).
 *
 * Conventions:
 *   - All voxel volumes are uint16, C-contiguous with X fastest:
 *     linear index = x + dims[0]*(y + dims[1]*z); dims = {nx, ny, nz}.
 *     (imglib2 dimension order: dim 0 = x.)
 *   - Affine matrices are row-major 3x4 double, mapping view-local (x,y,z,1)
 *     to world coordinates, identical to the reference's AffineTransform3D
 *     serialization (Spark.java:201-233: double[3][4]).
 *   - Caller owns every buffer. No exceptions cross the ABI; every entry
 *     point returns 0 on success or a negative BS_E* code. Thread-safe per
 *     context. Blocking; batching supplies parallelism.
 *   - A JNI binding for the stock Java host binds these symbols 1:1
 *     (see INTEGRATION.md).
 */
#ifndef BIGSTITCH_H
#define BIGSTITCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BS_OK 0
#define BS_EINVAL -1   /* bad argument */
#define BS_ENODEV -2   /* no HIP device / HIP error during init */
#define BS_ENOMEM -3   /* device or host allocation failed */
#define BS_EHIP -4     /* HIP runtime error mid-operation */
#define BS_ENOVIEW -5  /* view_id not uploaded */
#define BS_EUNSUP -6   /* unsupported parameter combination */

typedef struct bs_ctx bs_ctx;

/* Create a context bound to one HIP device (one context per GPU; work units
 * are hash-sharded across contexts by the host, mirroring the reference's
 * independent-RDD-element model — SURVEY.md §5 "no collectives"). */
int bs_ctx_create(bs_ctx **out, int device_id);
void bs_ctx_destroy(bs_ctx *ctx);

/* Last error message for a failed call on this ctx (valid until next call). */
const char *bs_last_error(const bs_ctx *ctx);

/* Free/total device memory of the ctx's GPU (host-side capacity
 * planning: the fusion CLI sizes its z-band view window from this). */
int bs_device_mem(bs_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* ------------------------------------------------------------------ views */

/* Upload a view's voxels to device HBM and register them under view_id.
 * Mirrors the reference's per-task image load (the N5 cell fetch behind
 * GroupedViewAggregator / ImgLoader). 288 GB HBM3E holds whole tile sets
 * resident; upload once, stitch/fuse many. */
int bs_view_upload(bs_ctx *ctx, int32_t view_id, const uint16_t *data,
                   const int64_t dims[3]);
int bs_view_release(bs_ctx *ctx, int32_t view_id);

/* Device-generated synthetic view (bench path only; BASELINE.json §(d)):
 * seeded Gaussian-blob content + noise floor. blob array is packed
 * {cx,cy,cz,sigma,amplitude} float5 per blob, positions in THIS view's
 * local coordinates (may lie outside [0,dims)). Overlapping blobs are
 * summed in fixed point, so the same arguments give a bit-identical view
 * on every call. */
int bs_view_synth(bs_ctx *ctx, int32_t view_id, const int64_t dims[3],
                  const float *blobs, int32_t n_blobs, uint32_t noise_seed,
                  uint16_t noise_floor, uint16_t noise_amp);

/* Download an uploaded/synth view back to host (tests). */
int bs_view_download(bs_ctx *ctx, int32_t view_id, uint16_t *out);

/* Optional per-view linear intensity coefficients for fusion
 * (reference SparkAffineFusion.java:545-559: Coefficients read per view
 * and applied inside BlkAffineFusion.initWithIntensityCoefficients).
 * ab: 2 * gx*gy*gz floats — the multiplicative plane (a), then the
 * additive plane (b), each a coarse grid covering the view uniformly;
 * the fusion kernel samples the grid trilinearly at cell centers
 * ([PIN-COEFF]) and applies value' = a*value + b before weighting.
 * Passing NULL clears the view's coefficients. */
int bs_view_set_coefficients(bs_ctx *ctx, int32_t view_id, const float *ab,
                             const int32_t grid_dims[3]);

/* View-group aggregation primitives (GroupedViewAggregator restatement
 * [PIN-GROUP]; reference SparkPairwiseStitching.java:204-208 applies
 * illumCombine then channelCombine over the {Illumination, Channel}
 * group of each Tile):
 *  - bs_view_combine_avg: out_id := voxelwise mean of n equal-sized
 *    uploaded views, rounded to nearest (ActionType.AVERAGE);
 *  - bs_view_sum: exact integer voxel sum (the host implements
 *    ActionType.PICK_BRIGHTEST by choosing the member with the highest
 *    mean = sum / voxels; exact u64 sums make the pick deterministic).
 */
int bs_view_combine_avg(bs_ctx *ctx, int32_t out_id, const int32_t *in_ids,
                        int32_t n);
int bs_view_sum(bs_ctx *ctx, int32_t view_id, uint64_t *sum);

/* --------------------------------------------------------------- stitching */

/* One tile-pair work unit. The overlap interval inside each view is computed
 * by the host from the current registrations exactly as the reference does
 * before calling computeStitching (PairwiseStitching operates on the
 * overlapping portions of the two grouped views). off/size are in view-local
 * full-resolution voxels, {x,y,z}. */
typedef struct {
  int32_t view_a, view_b;
  int64_t off_a[3], size_a[3];
  int64_t off_b[3], size_b[3];
} bs_pair_desc;

/* PairwiseStitchingParameters (reference SparkPairwiseStitching.java:200-202:
 * new PairwiseStitchingParameters(0, peaksToCheck(5), doSubpixel, ...);
 * downsampling flags :77 default {2,2,1}). */
typedef struct {
  int32_t ds[3];            /* downsample factors per axis, default {2,2,1} */
  int32_t peaks_to_check;   /* default 5 */
  int32_t do_subpixel;      /* default 1 */
  double min_overlap_ratio; /* min candidate overlap as fraction of the
                               smaller (downsampled) interval; default 0.25 */
  int32_t pad_mode;         /* [PIN-PAD] FFT pad size rule: 0 = next
                               power of two (this build's historical
                               default), 1 = next even 7-smooth "fast"
                               size (the imglib2 FFTMethods family the
                               reference's dependency uses) */
  int32_t _pad;             /* alignment */
} bs_stitch_params;

/* The result contract of computeStitching -> SerializablePairwiseStitchingResult
 * (Spark.java:201-233): a pure translation (3x4 with shift in last column),
 * correlation r, validity. shift[] is in FULL-RESOLUTION pixels of view
 * space, meaning: content of view B's interval matches content of view A's
 * interval displaced by +shift (B(x) ~ A(x - shift) over the overlap). */
typedef struct {
  double shift[3];
  double r;
  int32_t valid; /* 0: no peak passed the overlap test */
} bs_shift_result;

/* Padded FFT sizes ([PIN-PAD], of the downsampled intervals): x 8..1024,
 * y and z 1..1024 (pad_mode 1: 8..1024 on every axis, by its rule). A pair
 * outside that range fails the batch with BS_EUNSUP. A padded size of 1 on
 * y or z is supported and gives valid = 0, as in the reference restatement:
 * with periodic wrap a voxel is its own neighbour there, so the PCM has no
 * strict local maximum. */
int bs_stitch_batch(bs_ctx *ctx, const bs_pair_desc *pairs, size_t n,
                    const bs_stitch_params *params, bs_shift_result *out);

/* ------------------------------------------------------------------ fusion */

/* FusionType enum — reference SparkAffineFusion.java:124-125 (complete
 * except intensity-coefficient and --masks modes; CLOSEST_PIXEL_WINS
 * picks the view whose inverse-mapped point has the largest min-axis
 * distance to its view border [PIN], ties to the first view). */
#define BS_FUSION_AVG 0
#define BS_FUSION_AVG_BLEND 1
#define BS_FUSION_MAX_INTENSITY 2
#define BS_FUSION_LOWEST_VIEWID_WINS 3  /* first contributing view */
#define BS_FUSION_HIGHEST_VIEWID_WINS 4 /* last contributing view */
#define BS_FUSION_CLOSEST_PIXEL_WINS 5  /* largest border distance */

#define BS_OUT_FLOAT32 0
#define BS_OUT_UINT16 1
#define BS_OUT_UINT8 2

/* One input view participating in fusion. affine maps view-local to world
 * (bbox) coordinates; the library inverts it. Blend parameters mirror
 * mvrecon's Blending (border px, cosine ramp range px) used by
 * FusionType.AVG_BLEND. */
typedef struct {
  int32_t view_id;
  double affine[12]; /* row-major 3x4, view-local -> world */
  float blend_border[3];
  float blend_range[3];
} bs_fuse_view;

/* One output block: world-coordinate min and size ({x,y,z}), as produced by
 * Grid.create (reference SparkAffineFusion.java:459-461 — long[][]{offset,
 * size, gridPos}; gridPos is host-side bookkeeping, not part of the math). */
typedef struct {
  int64_t min[3];
  int64_t size[3];
} bs_block_desc;

typedef struct {
  int32_t fusion_type; /* BS_FUSION_*; reference default AVG_BLEND */
  int32_t out_dtype;   /* BS_OUT_*; conversion per RealUnsignedByte/Short
                          Converter min/max scaling (SparkAffineFusion.java:
                          497-517) */
  double min_intensity, max_intensity;
  int32_t interp; /* 1 = trilinear; only value supported (reference :611) */
  int32_t masks;  /* 1 = write coverage masks instead of fused intensities
                     (--masks; reference SparkAffineFusion.java:112-115,
                     :565-578 + fusion/GenerateComputeBlockMasks.java:
                     85-151): out = type max (uint8 255 / uint16 65535 /
                     float32 1.0) where ANY listed view's inverse affine
                     maps the voxel into [-mask_offset, dim-1+mask_offset]
                     per axis (inclusive), else 0. min/max_intensity
                     scaling does not apply. */
  double mask_offset[3]; /* --maskOffset, raw input px (default 0,0,0) */
} bs_fuse_params;

/* Fuse nb output blocks. views[] lists the views overlapping ANY of the
 * blocks; view_idx_per_block/view_idx_offsets give each block's culled view
 * list (the OverlappingViews.findOverlappingViews result, reference
 * fusion/OverlappingViews.java:28-47), as indices into views[].
 * out_blocks[i] receives prod(blocks[i].size) voxels of out_dtype. */
int bs_fuse_blocks(bs_ctx *ctx, const bs_fuse_view *views, size_t nviews,
                   const bs_block_desc *blocks, size_t nb,
                   const int32_t *view_idx_per_block,
                   const int64_t *view_idx_offsets, /* nb+1 prefix offsets */
                   const bs_fuse_params *params, void **out_blocks);

/* Volume-mode fusion + multi-resolution pyramid (SURVEY.md §8(f) row 1:
 * N5ApiTools.setupMultiResolutionPyramid / writeDownsampledBlock,
 * reference SparkAffineFusion.java:703-782, CreateFusionContainer.java:
 * 351-358). Fuses the whole bounding-box volume on-device (internal
 * block grid + OverlappingViews culling), then computes each pyramid
 * level from the previous by box-mean over the RELATIVE downsampling
 * factors (values rounded to nearest for integer dtypes), and stages
 * every level back into the caller's host buffers through pinned
 * double-buffering.
 *   abs_downsampling: nlevels x 3 ints, level 0 must be {1,1,1}; each
 *     level's factors must be integer multiples of the previous level's.
 *   level_dims_out (optional): nlevels x 3, receives ceil(dim/ds).
 *   level_buffers: caller-owned host buffers, one per level, each
 *     prod(level_dims)*dtype_size bytes. */
int bs_fuse_volume(bs_ctx *ctx, const bs_fuse_view *views, size_t nviews,
                   const int64_t vol_min[3], const int64_t vol_dims[3],
                   const bs_fuse_params *params, int32_t nlevels,
                   const int32_t *abs_downsampling, int64_t *level_dims_out,
                   void **level_buffers);

/* Debug-only: download the PCM volume of the LAST pair processed by
 * bs_stitch_batch on this ctx. out must hold prod(out_dims) floats; a
 * call with out=NULL only fills out_dims = {Px, Py, Pz}. Not part of the
 * drop-in surface; used by parity tooling.
 *
 * By default (environment variable BS_PCM_MODE=rows, read in
 * bs_ctx_create; forced to full by BS_PEAK_MODE=full) bs_stitch_batch
 * writes only the PCM rows its peak stage reads. bs_debug_pcm then first
 * rebuilds the whole volume from the pair's retained spectrum; it is
 * valid until the next bs_stitch_batch or bs_debug_peak_scan. */
int bs_debug_pcm(bs_ctx *ctx, float *out, int64_t out_dims[3]);

/* Debug-only: the same buffer without rebuilding it: under
 * BS_PCM_MODE=rows only the rows listed by bs_debug_rowlist belong to the
 * last pair, all other rows hold stale data. */
int bs_debug_pcm_raw(bs_ctx *ctx, float *out, int64_t out_dims[3]);

/* Debug-only: the PCM rows (index z*Py + y, unordered, no duplicates)
 * written for the LAST pair under BS_PCM_MODE=rows: the rows whose maximum
 * reaches the prefilter's threshold and their 8 periodic (y,z)
 * neighbours. At most cap entries are copied; *n receives their number
 * (0 when the pair's PCM was written whole). */
int bs_debug_rowlist(bs_ctx *ctx, int32_t *out, size_t cap, size_t *n);

/* Debug-only: the top five PCM maxima (value, linear index) of the LAST
 * pair processed by bs_stitch_batch, exactly as the candidate stage
 * received them. Missing entries carry the scan's sentinel
 * (v = -3e38, idx = INT64_MAX). */
int bs_debug_last_top5(bs_ctx *ctx, float v[5], int64_t idx[5]);

/* Debug-only: run the stitch path's peak stage on a caller-supplied
 * float volume (dims = {px, py, pz}, x fastest). mode 0 = auto (row-maxima
 * prefilter with the full scan as fallback), 1 = full scan. fell_back
 * (optional) receives 1 when the prefilter's result was rejected and the
 * full scan ran. The mode of bs_stitch_batch itself is fixed per context
 * by the environment variable BS_PEAK_MODE (auto | full) read in
 * bs_ctx_create. */
int bs_debug_peak_scan(bs_ctx *ctx, const float *pcm_host,
                       const int64_t dims[3], int mode, float v[5],
                       int64_t idx[5], int *fell_back);

/* Debug-only: run the context's r-test (the integer-sum cross-correlation
 * kernel of the candidate stage) on n <= 64 caller-chosen integer shifts
 * {sx, sy, sz} of one pair, at downsampling 1. Candidate boxes come from
 * the same function the candidate stage uses, without its min_overlap
 * filter; the launch is the candidate stage's own and is timed under
 * BS_K_CORR. sums_out[i] = {sum a, sum b, sum aa, sum bb, sum ab} over
 * the overlap of shift i and nvox_out[i] its voxel count (all zero when
 * the overlap is empty). Which kernel runs is fixed per context by the
 * environment variable BS_CORR_MODE (dot | wide | legacy) read in
 * bs_ctx_create. */
int bs_debug_rtest(bs_ctx *ctx, const bs_pair_desc *pair,
                   const int32_t (*shifts)[3], int n,
                   uint64_t (*sums_out)[5], int64_t *nvox_out);

/* -------------------------------------------- interest point detection */

/* Difference-of-Gaussian interest point detection on one uploaded view.
 * Replaces the in-process call site
 *   net.preibisch.mvrecon.process.interestpointdetection.methods.dog
 *       .DoGImgLib2.computeDoG(input, mask, sigma, threshold, localization,
 *           findMin, findMax, minIntensity, maxIntensity, blockSize, service,
 *           cuda = null, deviceCUDA = null, accurateCUDA, percentGPUMem)
 *     -> ArrayList<InterestPoint>
 * called from reference SparkInterestPointDetection.java:552-568. DoGImgLib2
 * is not part of the reference tree, so the arithmetic is this project's
 * restatement of the published method (Lowe 2004; Preibisch 2010), pinned by
 * tests/dog_ref.py; each restated constant carries a [PIN-*] tag:
 *   [PIN-DS2X]   residual downsample = float box mean over ds cells,
 *                output dims floor(n/ds) (trailing partial cell dropped)
 *   [PIN-SIGMA]  k = 2^(1/4), sigma2 = sigma*k, image sigma 0.5,
 *                s_i = sqrt(sigma_i^2 - 0.25), weight 1/(k-1)
 *   [PIN-GAUSS]  half size h = max(2, (int)(3 s + 0.5) + 1), taps
 *                exp(-x^2 / 2 s^2) over |x| <= h-1 normalised to unit sum,
 *                separable, mirror boundary with the edge sample repeated
 *   [PIN-DOG-SIGN] D = (G_s1 - G_s2) * weight: bright blob = positive maximum
 *   [PIN-EXTREMA] strict 26-neighbour extrema, all neighbours inside
 *   [PIN-THRESH] gate |D| >= threshold (NONE) or threshold/3 (QUADRATIC),
 *                then |fitted value| >= threshold
 *   [PIN-SUBPIX] iterative quadratic fit, at most 10 moves, accept when
 *                every |offset| <= 0.5 + 0.01*move
 * All arithmetic is float32 on the device except the per-candidate 3x3
 * solve, which is double. */
typedef struct {
  double sigma, threshold, min_intensity, max_intensity;
  int32_t find_min, find_max; /* --type MIN / MAX / BOTH */
  int32_t localization;       /* 0 NONE, 1 QUADRATIC */
  int32_t ds[3];              /* residual box-mean factors, powers of 2 */
} bs_dog_params;

typedef struct {
  double loc[3];     /* x,y,z in uploaded-view pixels: f*x + (f-1)/2 per
                        axis with residual factor f ([PIN-MIP]) */
  float value;       /* (fitted) DoG value */
  float intensity;   /* raw detection-scale input, trilinear at loc,
                        border clamped (reference :586-601) */
  int32_t kind;      /* +1 maximum, -1 minimum */
  int32_t converged; /* QUADRATIC: 1 if the fit was accepted, 0 if the point
                        is reported at its integer voxel; NONE: always 1 */
} bs_interest_point;

/* Detect on view_id. Writes min(*n_found, capacity) points — the first ones
 * in the order below — and always sets *n_found to the full count (out may
 * be NULL when capacity == 0; call twice to size the buffer). Points are
 * sorted by the linear index of their final integer voxel, maxima before
 * minima on a tie, then by the voxel they started from; the same arguments
 * give bit-identical arrays on every call.
 * Errors: BS_ENOVIEW unknown view; BS_EINVAL sigma <= 0.5, max_intensity ==
 * min_intensity, a ds factor that is not a power of two >= 1, neither
 * find_min nor find_max, localization not 0/1; BS_EUNSUP filter radius
 * h-1 > 32 or a detection-scale dim < 3; BS_ENOMEM when the float
 * temporaries (12 B/voxel, +4 with ds != 1) do not fit — the whole view is
 * processed at once. */
int bs_detect_dog(bs_ctx *ctx, int32_t view_id, const bs_dog_params *params,
                  bs_interest_point *out, size_t capacity, size_t *n_found);

/* Debug-only (parity tooling): the DoG volume D at detection scale, x
 * fastest. out_dims receives {nx,ny,nz} = floor(view dims / ds); with
 * out == NULL only the dims are returned. */
int bs_debug_dog_volume(bs_ctx *ctx, int32_t view_id,
                        const bs_dog_params *params, float *out,
                        int64_t out_dims[3]);

/* --------------------------------------------- interest point matching */

/* Geometric descriptor matching of two interest-point sets (the reference's
 * PRECISE_TRANSLATION method). Replaces the in-process call site
 *   net.preibisch.mvrecon...RGLDMPairwise.match(listA, listB)
 * constructed at reference SparkGeometricDescriptorMatching.java:594-604.
 * RGLDMPairwise is not part of the reference tree, so the arithmetic is this
 * project's restatement, pinned by tests/match_ref.py (tags [PIN-F32PTS],
 * [PIN-KNN], [PIN-RGLDM], [PIN-DESCDIST], [PIN-RATIO], [PIN-AMBIG] are
 * spelled out there). Device arithmetic is float32. */
typedef struct {
  int32_t num_neighbors;       /* n, default 3 */
  int32_t redundancy;          /* r, default 1 */
  float   ratio_of_distance;   /* --significance, default 3 */
  float   difference_threshold;/* default FLT_MAX */
  int32_t limit_search_radius; double search_radius;
} bs_match_params;
typedef struct { int32_t a, b; float best, second; } bs_match_candidate;

/* pts_a / pts_b: na / nb points, {x,y,z} double world coordinates. Writes
 * min(*n_found, capacity) candidates sorted by (a, b) and always sets
 * *n_found to the full count (out may be NULL when capacity == 0; call twice
 * to size the buffer). a / b index the input arrays; best / second are those
 * of the pair's descriptor match with the smallest best. A set with fewer
 * than n + r + 1 points gives zero candidates. The same arguments give
 * bit-identical arrays on every call.
 * Errors: BS_EUNSUP unless n >= 1, r >= 0, n + r <= 8, n <= 6, and when a
 * set has 2^31 descriptors or more; BS_EINVAL for a non-finite coordinate or
 * a negative search radius. */
int bs_match_descriptors(bs_ctx *ctx, const double *pts_a, size_t na,
                         const double *pts_b, size_t nb,
                         const bs_match_params *params,
                         bs_match_candidate *out, size_t capacity,
                         size_t *n_found);

/* Debug-only (parity tooling): k nearest neighbours of every point within
 * its set ([PIN-KNN]), 1 <= k <= 8. pts are rounded to float32 as given (no
 * minimum is subtracted: pass [PIN-F32PTS] values). idx_out int32 [n][k],
 * d2_out float [n][k]; with n <= k every entry is -1 / +inf. */
int bs_debug_ip_knn(bs_ctx *ctx, const double *pts, size_t n, int32_t k,
                    int32_t *idx_out, float *d2_out);

/* Debug-only: the raw result of the descriptor scan, one entry per A
 * descriptor (na * C of them, C = C(n + r, n); index = point * C + subset):
 * best, second (+inf where missing) and best_b (B descriptor index, -1 if
 * none). Nothing is written when either set has fewer than n + r + 1
 * points. The scan's split of B over the grid is chosen from the sizes;
 * the environment variable BS_IP_SPLIT (read in bs_ctx_create) forces a
 * number of slices, 1 = one scan per A descriptor. */
int bs_debug_ip_match(bs_ctx *ctx, const double *pts_a, size_t na,
                      const double *pts_b, size_t nb,
                      const bs_match_params *params, float *best_out,
                      float *second_out, int32_t *best_b_out);

/* Host-only RANSAC over correspondences ([PIN-RANSAC]; needs no context and
 * no GPU; csrc/bs_ransac.h). pa[i] <-> pb[i], {x,y,z} doubles; the model
 * maps A onto B: pb ~ M * (pa, 1), M row-major 3x4. */
#define BS_MODEL_NONE -1       /* regularizer only */
#define BS_MODEL_TRANSLATION 0
#define BS_MODEL_RIGID 1
#define BS_MODEL_AFFINE 2
#define BS_MODEL_IDENTITY 3    /* regularizer only */
typedef struct {
  int32_t model;            /* -tm, default AFFINE */
  int32_t regularizer;      /* -rm, default RIGID */
  double lambda;            /* default 0.1 */
  double max_epsilon;       /* -rme, default 5.0 */
  double min_inlier_ratio;  /* -rmir, default 0.1 */
  int32_t min_num_inliers;  /* -rmni, default 12 */
  int32_t iterations;       /* -rit, default 10000 */
} bs_ransac_params;

/* inlier_out (n bytes, optional) receives 1 for inliers; model_out
 * (optional) the model refitted on them; *n_inliers their count. Returns
 * BS_OK with *n_inliers = 0 (mask zero, model identity) when no consensus is
 * accepted. Deterministic: fixed seed, same input -> same output. */
int bs_ransac(const double *pa, const double *pb, size_t n,
              const bs_ransac_params *params, uint8_t *inlier_out,
              double model_out[12], size_t *n_inliers);

/* ----------------------------------------------------- intensity matching */

/* Pairwise intensity matching of two overlapping views. Replaces the
 * in-process call site
 *   net.preibisch.mvrecon...IntensityCorrection.matchRansac(data, v1, v2,
 *       renderScale, coefficientsSize, minThreshold, maxThreshold,
 *       minNumCandidates, iterations, maxEpsilon, minInlierRatio,
 *       minNumInliers, maxTrust)
 * of reference SparkIntensityMatching.java:173-174. IntensityCorrection is
 * not part of the reference tree, so the arithmetic is this project's
 * restatement, pinned by tests/intensity_ref.py; the tags [PIN-INT-GRID],
 * [PIN-INT-RENDER], [PIN-INT-CELL], [PIN-INT-RANSAC], [PIN-INT-TRUST] and
 * [PIN-INT-SOLVE] are spelled out in DESIGN.md "Intensity matching". Both
 * views are sampled on a coarse world grid; samples are quantised to integers P (view A) and
 * Q (view B) in 1/8 grey level and bucketed by the pair of coefficient
 * cells they fall in; each bucket gets a line Q = a P + b by RANSAC and
 * integer-moment refits. Every result is an integer or a fixed formula of
 * integers, so the same arguments give the same bits on every call. */
typedef struct {
  double render_scale;        /* --renderScale, in (0, 1], default 0.25 */
  int32_t coefficients[3];    /* --numCoefficients, cells per axis {x,y,z} */
  int32_t min_num_candidates; /* default 1000 */
  double min_threshold;       /* grey levels, default 1 */
  double max_threshold;       /* grey levels, NaN = none (default) */
  int32_t iterations;         /* 1 .. 4096, default 1000 */
  int32_t min_num_inliers;    /* default 10 */
  double max_epsilon;         /* grey levels, default 5.1 */
  double min_inlier_ratio;    /* default 0.1 */
} bs_intensity_params;

/* One accepted bucket. Moments are over the final inlier set, in units of
 * 1/8 grey level (sp = sum P, spq = sum P*Q, ...). a, b: Q/8 = a * P/8 + b,
 * b in grey levels; both follow from n_inl and the moments alone. */
typedef struct {
  uint64_t cell_a, cell_b;  /* linear cell ids, x fastest */
  uint64_t n_cand, n_inl;
  uint64_t best_it;         /* winning RANSAC iteration */
  uint64_t n_inl_first;     /* its inlier count, before any refit */
  uint64_t sp, sq, spp, sqq, spq;
  double a, b;
} bs_intensity_match;

/* Writes min(*n_found, capacity) buckets sorted by (cell_a, cell_b) and
 * always sets *n_found to the full count (out may be NULL when capacity ==
 * 0; call twice to size the buffer). affine_a / affine_b: row-major 3x4,
 * view-local -> world. Views whose transformed boxes do not intersect give
 * zero buckets and BS_OK.
 * Errors: BS_ENOVIEW unknown view; BS_EINVAL render_scale not in (0, 1], a
 * cell count < 1, iterations < 1, a singular affine; BS_EUNSUP more than
 * 65535 cells per view, more than 2^31 grid samples, a bucket above 2^24
 * members (the u64 moment bound), iterations > 4096. */
int bs_intensity_match_pair(bs_ctx *ctx, int32_t view_a,
                            const double affine_a[12], int32_t view_b,
                            const double affine_b[12],
                            const bs_intensity_params *params,
                            bs_intensity_match *out, size_t capacity,
                            size_t *n_found);

/* Debug-only (parity tooling): the render stage alone. grid_origin / grid_dims
 * receive g0 and dims of [PIN-INT-GRID] (dims all zero when the boxes are
 * disjoint); with p_out == NULL only they are returned. Otherwise p_out,
 * q_out (int32) and cell_a_out, cell_b_out (uint16) receive prod(dims)
 * samples, x fastest; invalid samples carry P = Q = -1. */
int bs_debug_intensity_render(bs_ctx *ctx, int32_t view_a,
                              const double affine_a[12], int32_t view_b,
                              const double affine_b[12],
                              const bs_intensity_params *params,
                              int64_t grid_origin[3], int64_t grid_dims[3],
                              int32_t *p_out, int32_t *q_out,
                              uint16_t *cell_a_out, uint16_t *cell_b_out);

/* Host-only global solve ([PIN-INT-SOLVE]; needs no context and no GPU;
 * csrc/bs_intensity_solve.h). Pair k joins views pair_views[2k] (its A
 * side) and pair_views[2k+1], indices in 0 .. nviews-1, and owns
 * matches[pair_offsets[k] .. pair_offsets[k+1]); only the integer fields of
 * a match are read. coeff_out: nviews * 2 * ncells doubles, per view the
 * multiplicative plane then the additive plane (grey levels), cells x
 * fastest — the layout bs_view_set_coefficients takes. iterations_out and
 * rel_residual_out are optional. Errors: BS_EINVAL for a cell count < 1, a
 * view index or cell id out of range, max_iterations < 1. */
typedef struct {
  double lambda_identity; /* default 0.01 */
  double lambda_smooth;   /* default 0.1 */
  int32_t max_iterations; /* default 1000 */
  int32_t _pad;
} bs_intensity_solve_params;

int bs_intensity_solve(int32_t nviews, const int32_t coefficients[3],
                       const int32_t *pair_views, const size_t *pair_offsets,
                       size_t npairs, const bs_intensity_match *matches,
                       const bs_intensity_solve_params *params,
                       double *coeff_out, int32_t *iterations_out,
                       double *rel_residual_out);

/* ------------------------------------------------------- instrumentation */

/* Per-kernel timing, HIP-event measured on the launch stream (bench.py
 * roofline evidence: average launch duration of the dominant kernel).
 * Accumulated since the last bs_reset_stats on this ctx. */
enum bs_kernel_id {
  BS_K_DOWNSAMPLE = 0,
  BS_K_FFT_X_FWD,  /* R2C load + x-line FFT */
  BS_K_FFT_Y_FWD,
  BS_K_FFT_Z_FWD,
  BS_K_FFT_Z_INV,  /* fused cross-power normalize + inverse z pass */
  BS_K_FFT_Y_INV,
  BS_K_FFT_X_INV,  /* inverse x pass + C2R (PCM write) */
  BS_K_PEAK,       /* PCM local-maxima top-5 tile scan */
  BS_K_PEAK_MERGE,
  BS_K_CORR,       /* candidate cross-correlation integer sums */
  BS_K_SUBPIX,     /* 7-point PCM gather */
  BS_K_FUSE,       /* inverse-affine trilinear blend fusion */
  BS_K_SYNTH,      /* bench-only synthetic tile render */
  BS_K_PYRAMID,    /* 2x (or general) box-mean pyramid level */
  BS_K_PEAK_ROWS,  /* peak prefilter chain (row maxima -> top five);
                      BS_K_PEAK/_MERGE then count only fallback scans */
  BS_K_DOG_XY,      /* fused x+y Gaussian passes, both sigmas (also counts
                       the residual box-mean launch when ds != 1) */
  BS_K_DOG_Z,       /* z pass for both sigmas + subtract + scale -> D */
  BS_K_DOG_EXTREMA, /* 3x3x3 strict extremum scan + gate + compaction */
  BS_K_DOG_SUBPIX,  /* per-candidate quadratic fit + intensity sample */
  /* intensity matching; placed ahead of the interest-point matching ids,
   * which stay the last three before BS_K_COUNT */
  BS_K_INT_RENDER,  /* both views sampled on the coarse world grid */
  BS_K_INT_MOMENTS, /* per-bucket integer moments (+ member compaction) */
  BS_K_INT_RANSAC,  /* per-bucket line hypotheses, inlier counts, arg-max */
  BS_K_IP_KNN,      /* brute-force k nearest neighbours within a point set */
  BS_K_IP_DESC,     /* descriptor gather */
  BS_K_IP_MATCH,    /* best / second descriptor scan (+ slice merge) */
  BS_K_COUNT
};

typedef struct {
  double total_ms[BS_K_COUNT];
  long long launches[BS_K_COUNT];
  double batch_ms;   /* whole-batch event-bracketed time (last batch) */
  long long pairs;   /* pairs processed since reset */
  long long blocks;  /* fusion blocks since reset */
} bs_batch_stats;

int bs_get_stats(bs_ctx *ctx, bs_batch_stats *out);
int bs_reset_stats(bs_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* BIGSTITCH_H */
