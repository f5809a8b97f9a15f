/*
 * modsx.h -- C ABI of the MI355X-native MODS inner loop (libmodsx.so).
 *
 * Every entry point replaces one interface of the reference (ducha-aiki/mods);
 * the file:line it replaces is cited on each declaration.  Plain pointers and
 * sizes only; no exceptions cross this boundary.  Conventions: an int return is
 * a count (>= 0) or a negative modsx_status; arrays returned through a `**`
 * parameter are malloc'd by the library and released with modsx_free(); device
 * state lives behind opaque handles; one modsx_ctx per calling thread (the
 * reference calls its detectors concurrently from nested OpenMP threads,
 * imagerepresentation.cpp:612-622 -- a ctx owns one HIP stream).
 *
 * The library needs a gfx950 device: modsx_create() fails (NULL +
 * modsx_last_error()) when none is present.  There is no CPU fallback.
 */
#ifndef MODSX_H
#define MODSX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MODSX_VERSION 100

typedef enum modsx_status {
  MODSX_OK = 0,
  MODSX_ERR_ARG = -1,
  MODSX_ERR_DEVICE = -2,
  MODSX_ERR_NOMEM = -3,
  MODSX_ERR_INTERNAL = -4,
  MODSX_ERR_CAPACITY = -5,  /* a caller-provided (or pooled) output buffer is too small: retry with a larger one */
  MODSX_ERR_TIMEOUT = -6    /* view-sharded path: a collective did not complete within the communicator's deadline (a peer rank
                               is missing or failed); the communicator is dead, destroy it and create a new one */
} modsx_status;

/* detection_mode_t, detectors/structures.hpp:11-15 */
enum { MODSX_FIXED_TH = 0, MODSX_RELATIVE_TH = 1, MODSX_FIXED_REG_NUMBER = 2, MODSX_RELATIVE_REG_NUMBER = 3,
       MODSX_NOT_LESS_THAN_REGIONS = 4 };
/* detector_type / descriptor_type, detectors/structures.hpp:17-38, 75-96 */
enum { MODSX_DET_HESSIAN = 0, MODSX_DET_DOG = 1, MODSX_DET_HARRIS = 2, MODSX_DET_MSER = 3 };   /* detector_type, detectors/structures.hpp:16-19 */
/* descriptor types of SIFTDescriptor::operator() (matching/siftdesc.cpp:399-442).  The half variants fold opposite
 * orientation bins into 64 values; their rows keep the 128 stride with entries 64..127 zero, which leaves every
 * L2 distance unchanged, so the matcher needs no second layout. */
enum { MODSX_DESC_SIFT = 0, MODSX_DESC_ROOT_SIFT = 1, MODSX_DESC_HALF_SIFT = 2, MODSX_DESC_HALF_ROOT_SIFT = 3 };
#define MODSX_MAX_DESC 4   /* descriptor classes one step can carry (the four SIFT-family types above) */
/* The real-valued descriptor classes of a stored representation (modsx_rep_append_f32 and what follows it).  They share the
 * namespace of modsx_rep_class_sel::desc_type; every entry that takes the types 0..3 alone goes on refusing them. */
enum { MODSX_DESC_CAFFE = 8, MODSX_DESC_DAISY = 9, MODSX_DESC_LIOP = 10, MODSX_DESC_MROGH = 11, MODSX_DESC_SURF = 12 };
/* The binary descriptor classes of a stored representation (modsx_rep_append_bin and what follows it), in the same namespace;
 * 4..7 and 13..15 stay unassigned.  Every entry that takes the types 0..3 alone, or 8..12, goes on refusing them. */
enum { MODSX_DESC_BRISK = 16, MODSX_DESC_FREAK = 17, MODSX_DESC_ORB = 18 };
enum { MODSX_DET_ORB = 4 };   /* detector_type DET_ORB, detectors/structures.hpp:20: a detector of binary classes only */
/* ScaleSpaceDetector point types, affinedetectors/pyramid.h:32-36 */
enum { MODSX_HESSIAN_DARK = 0, MODSX_HESSIAN_BRIGHT = 1, MODSX_HESSIAN_SADDLE = 2 };

/* == struct AffineKeypoint, detectors/structures.hpp:187-199 (same field order and layout) */
typedef struct modsx_keypoint {
  double x, y;
  double a11, a12, a21, a22;
  double s;
  double response;
  int octave_number;
  double pyramid_scale;
  int sub_type;
} modsx_keypoint;

/* == struct AffineRegion minus the heap-allocated Descriptor, detectors/structures.hpp:222-233.
 * Descriptors travel next to the region array as a dense [n][128] f32 matrix holding the
 * integers 0..255 the reference stores in Descriptor::vec (matching/siftdesc.cpp:218-274). */
typedef struct modsx_region {
  int img_id, img_reproj_id, id, parent_id, type;
  modsx_keypoint det_kp, reproj_kp;
} modsx_region;

/* PyramidParams + AffineShapeParams of ScaleSpaceDetectorParams,
 * detectors/structures.hpp:125-160, affinedetectors/affine.h:27-62, scale-space-detector.hpp:20-28 */
typedef struct modsx_hessaff_params {
  float threshold;
  int mode;
  int reg_number;
  float rel_threshold;
  float rel_reg_number;
  int numberOfScales;
  float initialSigma;
  double edgeEigenValueRatio;
  int border;
  int maxIterations;
  float convergenceThreshold;
  int smmWindowSize;
  float affInitialSigma;
  int doBaumberg;
  int detectorType;   /* PyramidParams::DetectorType (structures.hpp:148): MODSX_DET_HESSIAN (default), MODSX_DET_DOG or MODSX_DET_HARRIS --
                       * ScaleSpaceDetector::Response (pyramid.cpp:132-175), thresholds pyramid.h:47-67, point types pyramid.cpp:66-130 */
} modsx_hessaff_params;

/* scale-space keypoint before affine adaptation: the arguments of
 * KeypointCallback::onKeypointDetected, affinedetectors/pyramid.h:23-27 */
/* == struct extrema::ExtremaParams (the fields DetectMSERs reads), detectors/mser/extrema/extremaParams.h:49-82;
 * defaults of modsx_default_mser_params = [MSER] of build/config_iter_mods_cviu.ini:4-12 */
typedef struct modsx_mser_params {
  int min_size;          /* minimum region size in pixels */
  double max_area;       /* maximum region area relative to the image */
  double min_margin;     /* stability margin in grey levels (the detector threshold) */
  int relative;          /* margin relative to the grey level */
  int mode;              /* detection_mode_t, MODSX_FIXED_TH ... */
  int reg_number;
  float rel_threshold, rel_reg_number;
} modsx_mser_params;

typedef struct modsx_sskp {
  int octave, level, r0, c0, r, c, type, pad;
  float b0, b1, b2, val;
  float x, y, s, pixelDistance;
} modsx_sskp;

/* a localised 3x3x3 extremum as the scan kernels append it, before the detection order and the octaveMap claim
 * (modsx_debug_scan_levels) */
typedef struct modsx_candidate {
  int img, octave, level, type, r0, c0, r, c;
  float b0, b1, b2, val;
} modsx_candidate;

/* the fields MatchFlannFGINN fills in a TentativeCorrespExt (matching/matching.hpp:39-52):
 * first = list1[q], second = list2[t0], secondbad = list2[tj], secondbadby2ndcl = list2[t1] */
typedef struct modsx_tentative {
  int q, t0, tj, t1;
  double d1, d2, d2by2ndcl, ratio;
} modsx_tentative;

/* parameters of one identity-view HessAff -> SIFT -> FGINN -> LO-RANSAC pass over an image pair
 * (the body of mods.cpp:229-415 for one step); defaults = build/config_iter_mods_cviu.ini */
typedef struct modsx_pair_params {
  modsx_hessaff_params det;
  double ori_mrSize; int ori_patchSize; int ori_maxAngles; double ori_threshold; /* [DominantOrientation] :102-108 */
  double desc_mrSize; int desc_patchSize; int desc_photoNorm; int desc_type; double desc_maxBinValue; /* [SIFTDescriptor] :109-116 */
  double match_ratio; double contradDist; int nn;       /* FGINNThreshold, [Matching] contradDist :147 */
  double duplicateDist;                                  /* [DuplicateFiltering] :156-159, mode bestFGINN */
  double err_threshold, confidence; int max_samples; int localOptimization; double HLAFCoef; int doSymmCheck; /* [RANSAC] :162-170 */
  unsigned ransac_seed;
  int useF;            /* RANSACPars::useF (matching.hpp:148): 1 = epipolar verification, exp_ransacFcustom + F_LAF_check */
  double LAFCoef;      /* RANSACPars::LAFCoef, threshold of F_LAF_check = LAFCoef * err_threshold */
  int errorType;       /* RANSAC_error_t: 0 SAMPSON, 1 SYMM_MAX, 2 SYMM_SUM (F path: 1 and 2 both select FDsSym) */
  int detector;        /* MODSX_DET_HESSIAN (det) or MODSX_DET_MSER (mser): which detector the view loop runs */
  modsx_mser_params mser;
  /* The `Descriptors=` / `FGINNThreshold=` lists of one [DetectorN] section (iters_mods_cviu_wxbs.ini:35-36: RootSIFT,
   * HalfRootSIFT with 0.85, 0.8).  n_desc = 0: the one class {desc_type, match_ratio}.  n_desc = 1..4: the step carries these
   * descriptor classes, each matched with its own ratio; desc_type / match_ratio are then ignored.  See "descriptor classes"
   * at modsx_ladder_step. */
  int n_desc;
  int desc_types[MODSX_MAX_DESC];
  double desc_ratios[MODSX_MAX_DESC];
} modsx_pair_params;

typedef struct modsx_pair_result {
  int n_regions1, n_regions2;    /* described regions per image */
  int n_tentatives;              /* after MatchFlannFGINN */
  int n_unique;                  /* after DuplicateFiltering */
  int n_ransac_inliers;          /* exp_ransacHcustom inliers */
  int n_verified;                /* after NaiveHCheck + H_LAF_check */
  int ransac_samples, ransac_lo;
  double H[9];                   /* row-major, image 1 -> image 2 (LORANSACFiltering's H); with useF the
                                  * fundamental matrix as exp_ransacFcustom returns it */
  /* malloc'd arrays (modsx_free): tentatives after duplicate filtering in RANSAC order,
   * inlier flags from RANSAC, flags after the LAF check */
  modsx_tentative *tentatives;
  unsigned char *ransac_inlier;
  unsigned char *verified;
} modsx_pair_result;

/* == struct ViewSynthParameters (the geometric part), detectors/structures.hpp:201-214 */
typedef struct modsx_view {
  double zoom, tilt, phi, InitSigma;
  int doBlur;
} modsx_view;

typedef struct modsx_ctx modsx_ctx;
typedef struct modsx_image modsx_image;

int modsx_version(void);
const char *modsx_last_error(void);
void modsx_free(void *p);

/* With MODSX_MALLOC_TUNE=1 in the environment the first call also raises glibc's mmap / trim thresholds (mallopt) so that the
 * ~100 MB of host tables a pair allocates and frees stay mapped between calls (1 ms of page faults per 31-view pair otherwise).
 * Opt-in because it changes malloc for the whole host process. */
modsx_ctx *modsx_create(int device_id);
/* How the calling thread waits inside the calls that keep the device busy (MODSX_HOST_WAIT = runtime | flag | auto, default auto):
 * through hipStreamSynchronize, or by napping until a pinned flag word shows the sequence number that a one-lane kernel writes
 * behind the stage's launches (15 % less host CPU per pair, about 1 % fewer pairs/s when CPUs are plentiful, more pairs/s when they
 * are not).  `auto` takes the flag wait while the process uses more than 80 % of its CPU allowance (cgroup quota / local ranks).
 * A thread that naps there has its timer slack set to 2 us (prctl PR_SET_TIMERSLACK, once): its later sleeps wake on time. */
void modsx_destroy(modsx_ctx *ctx);
int modsx_synchronize(modsx_ctx *ctx);

void modsx_default_hessaff_params(modsx_hessaff_params *p);
void modsx_default_pair_params(modsx_pair_params *p);

/* Image upload.  dtype 0 = u8, 1 = f32; channels 1 or 3 (BGR as cv::imread gives).  3-channel input is
 * converted with the reference's (B+G+R)/3 rule: GenerateSynthImageCorr, synth-detection.cpp:253-262
 * (identity view: out_img.pixels = gray, :278-289). */
/* images are limited to 16384 px per side and 64 Mpx (32-bit pixel addressing in the samplers); larger ones are refused */
modsx_image *modsx_image_upload(modsx_ctx *ctx, const void *pixels, int rows, int cols, int channels, int dtype);
/* new pixels for an image made by modsx_image_upload, same size: no allocation (a caller that streams pairs through a context
 * keeps two images per context and refills them).  Synchronous like the upload: the buffer is the caller's again on return. */
int modsx_image_update(modsx_ctx *ctx, modsx_image *img, const void *pixels, int rows, int cols, int channels, int dtype);
/* wrap pixels that already live in HBM (f32, 1 channel, dense rows); not owned */
modsx_image *modsx_image_wrap_device(modsx_ctx *ctx, const float *dev_pixels, int rows, int cols);
void modsx_image_free(modsx_ctx *ctx, modsx_image *img);
int modsx_image_download(modsx_ctx *ctx, const modsx_image *img, float *out);

/* int DetectAffineKeypoints(cv::Mat &input, vector<AffineKeypoint> &out1, ScaleSpaceDetectorParams params,
 *                           ScalePyramid &scale_pyramid, const double tilt, const double zoom)
 * affinedetectors/scale-space-detector.hpp:231, .cpp:43-85 */
int modsx_detect_affine_keypoints(modsx_ctx *ctx, const modsx_image *img, const modsx_hessaff_params *par,
                                  double tilt, double zoom, modsx_keypoint **out);
/* stage tap: ScaleSpaceDetector::detectPyramidKeypoints without the affine callback (pyramid.cpp:540-573) */
int modsx_detect_scalespace(modsx_ctx *ctx, const modsx_image *img, const modsx_hessaff_params *par,
                            modsx_sskp **out);
/* stage tap: the 5 blur and 5 response levels of the first octave built from `img` as its first level
 * (ScaleSpaceDetector::detectOctaveKeypoints, pyramid.cpp:455-538); each output is 5*rows*cols f32 */
int modsx_octave_levels(modsx_ctx *ctx, const modsx_image *img, const modsx_hessaff_params *par, float *blurs,
                        float *resps);
/* stage taps for the two image primitives: gaussianBlur (detectors/helpers.cpp:717-724) and
 * cv::resize(.., 0.5, 0.5, INTER_LINEAR) (pyramid.cpp:520) */
int modsx_gaussian_blur(modsx_ctx *ctx, const modsx_image *img, float sigma, float *out);
int modsx_resize_half(modsx_ctx *ctx, const modsx_image *img, float *out, int *orows, int *ocols);

/* stage tap: Mat ScaleSpaceDetector::Response(const Mat &inputImage, float norm), affinedetectors/pyramid.cpp:132-175, for
 * DetectorType MODSX_DET_HESSIAN (HessianResponse :223-281), MODSX_DET_DOG (dogResponse :176-181: the input minus its
 * gaussianBlur with sigma = norm) and MODSX_DET_HARRIS (HarrisResponse :283-305: gradients, three blurred products,
 * det - 0.04 trace^2).  out: rows*cols f32.  The scale-space loop of modsx_detect_affine_keypoints itself runs the
 * Hessian response only (the shipped configurations use HessianAffine and MSER); the other two are provided as kernels. */
int modsx_response(modsx_ctx *ctx, const modsx_image *img, int detector_type, float norm, float *out);

/* template DetectAffineRegions<>: scale by sqrt|det A| and rectify, synth-detection.hpp:93-126 (host math) */
int modsx_detect_affine_regions(const modsx_keypoint *kps, int n, int img_id, int det_type, modsx_region *out);

/* int DetectMSERs(cv::Mat &input, std::vector<AffineKeypoint> &out1, extrema::ExtremaParams params,
 *                 ScalePyramid &scale_pyramid, const double tilt, const double zoom)
 *                                            detectors/mser/extrema/extrema.h:11, extrema.cpp:284-473 (doOnNormal)
 * MSER+ (sub_type 21) then MSER- (sub_type 20) of one view: x, y = centroid, A = covariance^(1/2), s = 1,
 * response = margin.  The view is truncated to u8 on the device; the component tree itself is sequential host code
 * (as in the reference).  Parity is pinned: tests/test_mser_ref_cpu.py and tests/test_gpu_mser_ref.py compare these entry points bit
 * for bit with the reference's own MSER sources, compiled in place for the tests (images of 64 pixels and more; smaller ones are
 * checked against the independent CPU restatement only).  *out is malloc'd (modsx_free).  Returns the number of keypoints. */
void modsx_default_mser_params(modsx_mser_params *p);
int modsx_detect_msers(modsx_ctx *ctx, const modsx_image *img, const modsx_mser_params *par, double tilt, double zoom,
                       modsx_keypoint **out);
/* the same on a host u8 image (what DetectMSERs builds at extrema.cpp:395-403); needs no device */
int modsx_detect_msers_u8(const unsigned char *gray, int rows, int cols, const modsx_mser_params *par, double tilt,
                          double zoom, modsx_keypoint **out);

/* int DetectOrientation(AffineRegionList &in, AffineRegionList &out, SynthImage &img, double mrSize,
 *                       int patchSize, int doHalfSIFT, int maxAngNum, double th, bool addUpRight)
 * synth-detection.hpp:151-159, .cpp:841-919 */
int modsx_detect_orientation(modsx_ctx *ctx, const modsx_image *img, const modsx_region *in, int n, double mrSize,
                             int patchSize, int doHalfSIFT, int maxAngNum, double th, int addUpRight,
                             modsx_region **out);

/* int ReprojectRegions(AffineRegionList &keypoints, double *H, int orig_w, int orig_h)
 * synth-detection.cpp:541-616; filters in place, returns the new count (host math) */
int modsx_reproject_regions(modsx_region *regs, int n, const double *H, int orig_w, int orig_h);
/* int ReprojectRegionsAndRemoveTouchBoundary(AffineRegionList &keypoints, double *H, int orig_w, int orig_h,
 *                                            const double mrSize = 3.0*sqrt(3.0))        synth-detection.cpp:63-102, .hpp:68
 * The same with the box mrSize * s instead of k_sigma * s: the un-oriented "None" list SynthDetectDescribeKeypoints keeps
 * beside the described ones (imagerepresentation.cpp:1271-1272; what SaveRegions writes for regions without descriptors). */
int modsx_reproject_regions_touch_boundary(modsx_region *regs, int n, const double *H, int orig_w, int orig_h, double mrSize);

/* template DescribeRegions<SIFTDescriptor>(AffineRegionList&, SynthImage&, FuncType, double mrSize,
 *            int patchSize, bool fast_extraction, bool photoNorm)     synth-detection.hpp:169-255
 * with SIFTDescriptor::operator() matching/siftdesc.cpp:401-442.  desc: n*128 f32 (integers 0..255). */
int modsx_describe_regions(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                           int patchSize, int fast_extraction, int photoNorm, int desc_type, double maxBinValue,
                           float *desc);

/* int MatchFlannFGINN(const AffineRegionList &list1, const AffineRegionList &list2,
 *                     TentativeCorrespListExt &corresp, const MatchPars &par, const int nn = 50)
 * matching/matching.hpp:268-269, .cpp:357-461 with vector_matcher = linear, vector_dist = L2.
 * desc*: [n][128] f32 holding integers 0..255 (anything else -- fractions, out-of-range values, NaN -- is refused with
 * MODSX_ERR_ARG: the int8 matrix-core path is exact only on that domain); pos2: [n2][2] reproj_kp x,y of list2.
 * A ratio >= 1 takes the reference's "all points" branch (matching.cpp:397-428): a record per query, closed by its first
 * contradictive neighbour or by neighbour nn - 1 (no ratio test).
 * nn must lie in [2, 256] (the reference takes any nn, default 50; the device walk lists fewer than nn groups of trains per
 * query, in 256 slots): other values return MODSX_ERR_ARG on every match path, the sharded and fused ones included.
 * Images must have at least 2 rows and 2 columns (modsx_image_upload / modsx_image_wrap_device refuse smaller ones). */
int modsx_match_fginn(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, const double *pos2,
                      double ratio, double contradDist, int nn, modsx_tentative **out);

/* void DuplicateFiltering(TentativeCorrespListExt&, const double r, const int mode) matching/matching.hpp:300,
 * .cpp:2983-3047.  pts: [T][4] = x1 y1 x2 y2; key: |ratio| (bestFGINN), d1 or scale; order[] receives the
 * permutation of the sort, keep[] the survivor flags in sorted order.  Returns the survivor count. */
int modsx_duplicate_filtering(const double *pts, const double *key, int T, double r, int do_sort, int *order,
                              unsigned char *keep);

/* Score exp_ransacHcustom(double *u, int len, double th, double conf, int max_sam, double *H,
 *          unsigned char *inl, int iter_type, int *data_out, int oriented_constraint, unsigned inlLimit,
 *          double **resids, HDsPtr, HDsiPtr, HDsidxPtr, int doSymCheck)       degensac/exp_ranH.h:29-36
 * with the Sampson error functions (HDs/HDsi/HDsidx) and iter_type 4, plus an explicit seed in place of
 * srand(time(NULL)) (exp_ranH.c:823).  u: [len][6] = x1 y1 1 x2 y2 1; H: column-major-as-returned (maps
 * image 2 -> image 1 transposed, see matching.cpp:922-938); data_out[0..2] = samples, LO count, orientation
 * rejects.  Returns the inlier count. */
int modsx_ransac_h(const double *u, int len, double th, double conf, int max_sam, double *H, unsigned char *inl,
                   int *data_out, int oriented_constraint, int doSymCheck, unsigned seed, double *score_J);

/* int LORANSACFiltering(TentativeCorrespListExt &in, TentativeCorrespListExt &out, double *H,
 *                       const RANSACPars pars)   matching/matching.hpp:284-286, .cpp:806-980 (useF = 0,
 * errorType SAMPSON).  pts [T][4]; laf1/laf2 [T][5] = reproj a11 a12 a21 a22 s.  Outputs H (row-major
 * img1->img2), Hraw (as exp_ransacHcustom returned it), inl (RANSAC), keep (after NaiveHCheck + H_LAF_check).
 * Returns the verified count. */
int modsx_loransac_h(const double *pts, const double *laf1, const double *laf2, int T, double err_threshold,
                     double confidence, int max_samples, int localOptimization, double HLAFCoef, int doSymmCheck,
                     unsigned seed, double *H, double *Hraw, unsigned char *inl, unsigned char *keep,
                     int *data_out);

/* The same two calls with RANSACPars::errorType (matching.cpp:821-846 picks the HDS1 / HDSi1 / HDSidx1 triple the whole
 * of exp_ransacHcustom scores with): 0 SAMPSON = HDs, 1 SYMM_MAX = HDsSymMax, 2 SYMM_SUM = HDsSym (the RANSACPars
 * default, matching.hpp:138-171).  modsx_ransac_h / modsx_loransac_h are error_type 0; modsx_pair_params.errorType
 * selects it for the fused callers. */
int modsx_ransac_h_errtype(const double *u, int len, double th, double conf, int max_sam, double *H, unsigned char *inl,
                           int *data_out, int oriented_constraint, int doSymCheck, int error_type, unsigned seed,
                           double *score_J);
int modsx_loransac_h_errtype(const double *pts, const double *laf1, const double *laf2, int T, double err_threshold,
                             double confidence, int max_samples, int localOptimization, double HLAFCoef, int doSymmCheck,
                             int error_type, unsigned seed, double *H, double *Hraw, unsigned char *inl,
                             unsigned char *keep, int *data_out);

/* int exp_ransacFcustom(double *u, int len, double th, double conf, int max_sam, double *F, unsigned char *inl,
 *                       int *data_out, int do_lo, unsigned inlLimit, double **resids, double *H_best, int *Ih,
 *                       exFDsPtr EXFDS1, FDsPtr FDS1, int doSymCheck)      degensac/exp_ranF.c:795-1192
 * LO-RANSAC + DEGENSAC (plane-and-parallax) for the fundamental matrix; u [len][6] = x1 y1 1 x2 y2 1, th squared.
 * error_type 0 = Sampson (FDs/exFDs), 1 = symmetric epipolar distance (FDsSym/exFDsSym), matching.cpp:821-846.
 * F: 9 doubles as the reference returns them (x2^T F x1 = 0 with F read row-wise).  data_out: samples drawn,
 * local optimisations, degenerate (H-consistent) samples handled.  `seed` replaces srand(time(NULL)).
 * Returns the inlier count of the best model. */
int modsx_ransac_f(const double *u, int len, double th, double conf, int max_sam, int do_lo, unsigned inl_limit,
                   int error_type, int doSymCheck, unsigned seed, double *F, unsigned char *inl, int *data_out);

/* LORANSACFiltering with RANSACPars::useF = 1 (matching.cpp:806-980): exp_ransacFcustom + F_LAF_check (:193-250,
 * threshold LAFCoef * err_threshold).  Same argument layout as modsx_loransac_h.  Returns the verified count. */
int modsx_loransac_f(const double *pts, const double *laf1, const double *laf2, int T, double err_threshold,
                     double confidence, int max_samples, int localOptimization, double LAFCoef, int doSymmCheck,
                     int error_type, unsigned seed, double *F, unsigned char *inl, unsigned char *keep, int *data_out);
/* The hypothesis loop of DEGENSAC's plane-and-parallax step (rFtH, DegUtils.c:254-440: up to 2 x 10^4 two-point epipoles per
 * H-degenerate sample, each scored with FDs over the off-plane correspondences) runs on the device when the calling thread has
 * one: the host draws the samples of a batch from a copy of the PRNG, one device thread per hypothesis counts, the host acts on
 * the first count that changes the loop's state exactly as the reference does.  Same trajectory, same F (tests/test_gpu_verify.py
 * against the reference's compiled degensac).  MODSX_VERIFY_DEVICE=0 keeps the loop on the host; without a device it is there
 * anyway.  A device state that failed to set up, hit a HIP error or disagreed with the host's recount is torn down, the loop at
 * hand finishes on the host, and the next loop starts a fresh state; after 8 such failures in a process the loops stay on the host.  out[0..6): device batches, hypotheses counted on the device, state-changing hypotheses, host / device disagreements,
 * rFtH loops run (either way) and the microseconds they took (process-wide; reset != 0 clears them).  Returns 6. */
int modsx_verify_device_stats(long *out, int reset);
/* out[0..4): microseconds of those loops spent drawing samples ahead of a batch, waiting for the device, in the host phase
 * (hypotheses that changed nothing, counted on the host at the start of a loop and after every state change) and in the bodies of
 * state-changing hypotheses.  Process-wide; reset != 0 clears them.  Returns 4. */
int modsx_verify_device_timing(long *out, int reset);

/* One step of mods.cpp's iteration loop (:229-415) for an identity view: detect + orient + describe both
 * images, match, filter duplicates, verify.  Images and all intermediates stay in HBM between stages. */
int modsx_match_pair(modsx_ctx *ctx, const modsx_image *img1, const modsx_image *img2,
                     const modsx_pair_params *par, modsx_pair_result *res);
void modsx_pair_result_release(modsx_pair_result *res);

/* A batch of independent pairs, pipelined over n_ctx contexts (one host thread + one HIP stream each), the
 * counterpart of the reference's OpenMP parallelism over images / views (mods.cpp:255-271,
 * imagerepresentation.cpp:612-622): host-side bookkeeping of one pair overlaps device work of another.
 * Every context takes up to 4 pairs at a time and runs their 8 images as one launch set; DuplicateFiltering +
 * LO-RANSAC of a finished group run on helper threads (one per working context) while the context's thread feeds
 * the next group to its stream.  Results are those of n_pairs modsx_match_pair calls.
 * All contexts must live on the device that holds the images.  Returns n_pairs. */
int modsx_match_pairs(modsx_ctx *const *ctxs, int n_ctx, const modsx_image *const *imgs1,
                      const modsx_image *const *imgs2, int n_pairs, const modsx_pair_params *par,
                      modsx_pair_result *results);

/* The same for multi-view pairs (mods.cpp's loop over image pairs with one view list per image, as modsx_match_pair_views
 * per pair): every context takes one pair at a time off a shared counter; DuplicateFiltering + LO-RANSAC of a matched pair
 * run on helper threads while the context goes on to the next pair.  Results are those of n_pairs modsx_match_pair_views
 * calls.  Returns n_pairs. */
int modsx_match_pairs_views(modsx_ctx *const *ctxs, int n_ctx, const modsx_image *const *imgs1,
                            const modsx_image *const *imgs2, int n_pairs, const modsx_view *views, int n_views,
                            const modsx_pair_params *par, modsx_pair_result *results);

/* host share of the process's last batch call: wall time of DuplicateFiltering + LO-RANSAC summed over its pairs (ms), the pairs
 * verified and the contexts that worked on the call, min(n_ctx, groups), each with a helper thread (measurement hook).  Written by
 * all four batch entries: modsx_match_pairs, modsx_match_pairs_views, modsx_match_reps, and modsx_match_one_to_many, which leaves
 * the values of the last round of its ladder.  The same holds for modsx_debug_last_batch_verify_each and
 * modsx_debug_last_batch_cpu.  A failed call leaves the values of the part that ran */
int modsx_last_batch_verify(double *sum_ms, int *pairs, int *threads);
/* shape of the process's most recent matcher launch, as used for its first problem: 32-query sets per wavefront (2 / 4), whole-CU
 * workgroups (0 / 1), splits of the train tiles, tiles per split, upper bound of the tile count (measurement hook).  The five
 * values are written one by one: they belong together only while a single thread launches matcher work */
int modsx_last_match_geometry(int *qs, int *fat, int *S, int *tiles_per_split, int *ntiles_ub);
/* what the description stage planned on this context since modsx_create, cumulative (measurement hook); the contexts that work on
 * its behalf (the peer of a lone multi-view pair, the chains of contexts that take parts of a view list) count with it.  Fills
 * out[0 .. min(n, 15) - 1] and returns 15.  In order: description calls; chunks (launch sets, cut where the window arena of
 * MODSX_ARENA_MB is full); the largest number of chunks in one call; chunks that began in the middle of an image's region list;
 * chunks that began at an image other than the call's first; regions; regions of the direct branch (no smoothed window); windows
 * whose sampling kernel also ran the column filter; row tiles and column tiles of the LDS filters; tiles of the global-memory
 * sampling kernel, of the global-memory row filter and of the global-memory column filter; windows whose LDS row tile was clamped
 * to 32 rows; and, last, ordered_workgroups: the k_describe workgroups (SIFT and raw-histogram forms; two regions each, DESIGN.md
 * section 6.6) that took the ordered gather instead of the order-free one.  That one is counted on the device, which the planner
 * cannot know: modsx_debug_describe_plan fills the first 14 only, and this call waits for the context's stream and copies
 * the word (the description calls do neither for it).  A call is counted when its planning begins and a chunk when its walk begins: a call refused for a window that is
 * too large counts as one call and one chunk with no regions and leaves the largest-chunks value alone, and a call without any
 * region counts as a call with no chunk.  Read it while no call runs on the context; tests work with the difference of two
 * readings */
int modsx_describe_counters(modsx_ctx *ctx, long *out, int n);
/* Measurement hook: which form of the SIFT describe kernel the launch sets of a context (and of those that describe on its behalf)
 * took since modsx_create: out[0 .. min(n, 3) - 1], returns 3.  In order: launch sets that took the slim form (one LDS buffer per
 * region) with its redo launch -- those without a direct-branch region, unless MODSX_DESCRIBE_SLIM=0 was set when the context was
 * created --; launch sets that took the full kernel; and redo workgroups: the slim form's workgroups that needed the ordered
 * gather and were run again by the redo launch (each also counts in ordered_workgroups).  The last is counted on the device:
 * the call waits for the context's stream, like modsx_describe_counters */
int modsx_describe_slim_counters(modsx_ctx *ctx, long *out, int n);
/* Test entries and measurement hooks of the scale-space front end (ScaleSpaceDetector, affinedetectors/pyramid.cpp).
 * modsx_blur_geometry (host only): the tile rule of the pyramid's blur launch over n planes of rows[i] x cols[i] (1 <= n <= 32):
 * geometry[0] = rows of a 64-column tile, 32 when the launch has at least 2560 such tiles and 16 otherwise; geometry[1] = the
 * tiles (workgroups) of the launch.  The launcher calls the same function.
 * modsx_detect_counters: what the front end launched on this context since modsx_create (host-side counts; the contexts that
 * work on its behalf count with it in the cumulative entries).  Fills out[0 .. min(n, 19) - 1] and returns 19.  In order: blur
 * launches with 16-row and with 32-row tiles; blur launches by instantiated half width R = 1 .. 8 (8 entries; ksize = 2 R + 1);
 * launches of the stand-alone Hessian kernel; of the resize (+ Hessian) kernel; extrema scan launches that number their tiles
 * per octave (numberOfScales = 3) and per level (every other count, or MODSX_NMS_PER_LEVEL in the environment); scan launches
 * made because the table of 1024 (image, octave, level) jobs was full, i.e. before a scan's last launch; then, of the context's
 * LAST scan: its jobs and its tiles over all its launches; the accepted candidates of the last candidate set that was
 * downloaded; and (cumulative again) downloads that had to copy the records a second time because the set held more than the
 * speculative copy (the previous set's count + 1/4 + 1024).  Read it while no call runs on the context; tests work with the
 * difference of two readings.
 * modsx_debug_pyramids: builds the pyramids of a batch of n <= 32 images (sizes may differ) as modsx_detect_scalespace does.
 * geometry[49 i] = octaves of image i, geometry[49 i + 1 + 2 o], [.. + 2 + 2 o] = rows, cols of its octave o; *need_floats =
 * the floats of all planes.  planes = NULL: geometry and size only, nothing is launched.  Otherwise planes (cap_floats floats)
 * receives image after image, octave after octave, the numberOfScales + 2 blur planes and then as many response planes.
 * modsx_debug_scan_levels: the production extrema scan, detection order and octaveMap claim on the L = numberOfScales + 2
 * response and blur planes (each L * rows * cols f32) of ONE octave supplied by the caller (octave 0, pixelDistance 1, sides
 * below 16384).  *cands / *n_cands: the accepted records as the device appended them, in no particular order; the return value
 * and *out: the keypoints after the order and the claim.  Both arrays are released with modsx_free.
 * modsx_debug_detect_scalespace_batch: modsx_detect_scalespace for n <= 32 images in ONE launch set; out[i] / counts[i] per image.
 * All of them refuse border < 1 (MODSX_ERR_ARG), as every detection entry does: the scan would read before the planes. */
int modsx_blur_geometry(const int *rows, const int *cols, int n, int *geometry);
int modsx_detect_counters(modsx_ctx *ctx, long *out, int n);
int modsx_debug_pyramids(modsx_ctx *ctx, const modsx_image *const *imgs, int n, const modsx_hessaff_params *par, int *geometry,
                         float *planes, unsigned long long cap_floats, unsigned long long *need_floats);
int modsx_debug_scan_levels(modsx_ctx *ctx, const float *resps, const float *blurs, int L, int rows, int cols,
                            const modsx_hessaff_params *par, modsx_candidate **cands, int *n_cands, modsx_sskp **out);
int modsx_debug_detect_scalespace_batch(modsx_ctx *ctx, const modsx_image *const *imgs, int n, const modsx_hessaff_params *par,
                                        modsx_sskp **out, int *counts);
/* The device half of DetectMSERs in the view loop, for one launch set of 1 <= n <= 32 views (views_host[i]: rows[i] x cols[i]
 * f32 on the host, any rows, cols >= 1, sizes may differ; copied to device scratch as they are): the views go through the
 * function the loop itself calls -- u8 truncation, (unsigned char)float as x86 evaluates it, and the stable counting sort by grey
 * level, device sort on -- and come back as downloaded.  u8 and order receive view after view (rows x cols bytes / ints each;
 * order = the offsets (r + 1) * (cols + 2) + c + 1 of the view's pixels by (grey level, raster position)), start the n x 257
 * level starts (start[257 i + l] = pixels of view i below level l, [257 i + 256] = its pixels).  MODSX_ERR_ARG for anything else */
int modsx_debug_mser_front(modsx_ctx *ctx, const float *const *views_host, const int *rows, const int *cols, int n,
                           unsigned char *u8, int *start, int *order);
/* orientation jobs launched by the pair and view pipelines of this process, and regions they left out of the orientation launch
 * because modsx_debug_reproject_certain_drop flags them, since the last reset (measurement hook; MODSX_ORI_PREFILTER=0 in the
 * environment launches them all).  modsx_detect_orientation itself never leaves a region out */
int modsx_debug_orientation_counts(unsigned long long *launched, unsigned long long *skipped, int reset);
/* launches of the orientation kernel by every context of this process since the last reset (measurement hook), by instance:
 * *lds_table the launches that read the bin table from a copy in LDS (fewer than 8192 regions), *global_table those that read it
 * in global memory.  modsx_detect_orientation and the pipelines count alike; a call with no region to orient launches nothing.
 * Either pointer may be NULL.  Returns 0 */
int modsx_debug_orientation_launches(unsigned long long *lds_table, unsigned long long *global_table, int reset);
/* view synthesis by every context of this process since the last reset (measurement hook): *views_fused the non-identity views
 * that went source image -> view in the one fused launch, *groups the groups of shared rotations they formed (views of one
 * launch set whose source image, sizes and inverse rotation match bit for bit are rotated once; MODSX_VIEWS_SHARE_ROT=0 in the
 * environment makes every view a group of its own), *rotated_pixels the sum of w_rot x h_rot over those groups.  Any pointer may
 * be NULL.  Returns 0 */
int modsx_debug_views_counters(unsigned long long *views_fused, unsigned long long *groups, unsigned long long *rotated_pixels,
                               int reset);
/* host only (no device, no context): the plan of one view of a rows x cols image.  geometry[8] = {is_identity, w_rot, h_rot,
 * out_cols, out_rows, kx, ky, kind}, kind = 2: the fused launch, 1: rotate + blur fused and a second launch for the tilt,
 * 0: one launch per stage (what the environment of the process selects; an identity view has kind 0); rinv[6] / winv[6]
 * (optional) = the inverse maps of the rotation and of the tilt / zoom as the kernels receive them.  Returns 0 or an error */
int modsx_debug_view_plan(int rows, int cols, const modsx_view *view, int *geometry, double *rinv, double *winv);
/* host only: the grouping rule of the fused launch on n views given by their plans.  source[i] tells source images apart,
 * dims[5 i ..] = {source rows, source cols, h_rot, w_rot, kind}, rinv[6 i ..] the inverse rotation.  cap <= 0: the built-in
 * cap.  group[i] = the view's group in job-table order, -1 for a view that does not take the fused launch (kind != 2);
 * order[n] = the views in job-table order; totals[5] = {views fused, groups, tiles, rotated pixels, rotated pixels without
 * sharing}.  Returns 0 or an error */
int modsx_debug_views_groups(const int *source, const int *dims, const double *rinv, int n, int cap, int *group, int *order,
                             long long *totals);
/* the n <= 32 (image, view) items synthesised as ONE launch set, the way the view loops of the pipelines do it (measurement and
 * test hook; modsx_synth_view is the same for n = 1).  out[i]: a new image handle (modsx_image_free); is_identity[i] = 1: the
 * handle aliases imgs[i].  Returns 0 or an error (no handle is left behind then) */
int modsx_debug_synth_views(modsx_ctx *ctx, const modsx_image *const *imgs, const modsx_view *views, int n, modsx_image **out,
                            int *is_identity);
/* host only: the tables the orientation kernel reads, built by the function that fills a context's copies.
 * bin_table [2049]: the histogram bin (int)(36 * (angle / pi + 1) / 2) of the atan2LUTff angle of case code * 256 + idx, code =
 * (x > 0) << 2 | (y > 0) << 1 | (|x| > |y|), idx = (int)(255 * small / big) clamped to 0 .. 255; entry 2048 is the special case
 * x == 0, y <= 0 (angle 0).
 * index_raster / weight_raster [1344]: the pixels of the 41 x 41 patch that can vote (circular mask of sigma 41 / 3 above 0) in
 * raster order, as row * 44 + column, and their mask values; entries from counts[0] on are padding (pixel 45, weight 0).
 * index_lanes / weight_lanes [1344]: the same list as the kernel reads it, entry lane + 64 q = raster entry 21 lane + q.
 * counts [4]: voting pixels (1245), list length (1344), row stride of the indices (44), the region count from which a launch
 * reads the bin table in global memory (8192).  Any pointer may be NULL.  Returns 0 */
int modsx_orientation_tables(unsigned char *bin_table, unsigned short *index_raster, float *weight_raster,
                             unsigned short *index_lanes, float *weight_lanes, int *counts);
/* drop[i] = 1 when modsx_reproject_regions (boxk = 2 * 3 * sqrt 3) / modsx_reproject_regions_touch_boundary (boxk = mrSize) with
 * the same H and size removes region i whatever rotation modsx_detect_orientation applies to its shape first, 0 when that is not
 * certain (host only).  Returns n */
int modsx_debug_reproject_certain_drop(const modsx_region *regs, int n, const double *H, int orig_w, int orig_h, double boxk,
                                       unsigned char *drop);
/* The description stage's plan of one call, without a device and without a context (host only; measurement hook): the region
 * lists of `nimages` images (regs: one flat array, counts[i] regions of image i; modsx_describe_regions is nimages = 1) planned
 * for mr_size and fast_extraction with a window arena of arena_floats floats (MODSX_ARENA_MB << 18).  counters[0 .. min(n, 14) - 1]
 * get what modsx_describe_counters of a fresh context shows after that one call; cuts[0 .. min(*n_cuts, cap_cuts) - 1] the flat
 * index of the first region of every chunk after the first, *n_cuts their number.  Returns MODSX_OK, or the call's refusal
 * (MODSX_ERR_ARG and its modsx_last_error text) with the counters as the refused call leaves them */
int modsx_debug_describe_plan(const modsx_region *regs, const int *counts, int nimages, double mr_size, int fast_extraction,
                              unsigned long long arena_floats, long *counters, int n, long *cuts, int cap_cuts, int *n_cuts);
/* The same walk, reporting per chunk whether it may take the slim form of the describe kernel (no region of the direct branch):
 * slim[0 .. min(*n_chunks, cap) - 1], *n_chunks the chunks planned.  Host only */
int modsx_debug_describe_plan_slim(const modsx_region *regs, const int *counts, int nimages, double mr_size, int fast_extraction,
                                   unsigned long long arena_floats, unsigned char *slim, int cap, int *n_chunks);
/* Test entries of the Baumberg stage (AffineShape::findAffineShape, affinedetectors/affine.cpp:26-169).
 * modsx_debug_baumberg_geometry (host only): what a launch of n keypoints at window W runs, geometry[4] = kernel (0 = the
 * two-slot stream kernel on static chunks, 1 = the one-keypoint kernel with the window size compiled in, 2 = the one-keypoint
 * kernel for any window), keypoints per wavefront, wavefronts with work, workgroups.  variant 0 = the stream kernel on static
 * chunks where there is one (W = 19), else kernel 1 / 2; 1 = kernel 1 (W = 19 only), 2 = kernel 2 (odd W in 3..19); chunk 0 =
 * the production rule, otherwise the keypoints per wavefront of the stream kernel (>= 1).  variant 3 (W = 19 only) = the stream
 * kernel fed from a launch-wide queue, geometry[4] = kernel 3, wavefronts per range of the job list, ranges (8), workgroups
 * (8 x wavefronts per range); chunk > 0 = that many wavefronts per range (<= 2^20).  Its production rule, chunk 0, is one
 * resident set of wavefronts of the launching context's device (never more than ceil(n / 2), rounded up to a multiple of 8):
 * the host-only entry does not know a device and refuses it, modsx_debug_baumberg_geometry_ctx answers for a context (which
 * asks the runtime once).  MODSX_ERR_ARG (kernel -1) where there is no such launch.
 * modsx_debug_baumberg_variant (host only): the variant modsx_detect_affine_keypoints launches at window W: 3 at W = 19, else
 * 0.  MODSX_BAUMBERG_QUEUE in the environment (read once per process) overrides it for A/B runs: 0 = always variant 0, another
 * number = variant 3 at W = 19.
 * modsx_debug_baumberg: runs that launch on the context's stream for a job list -- job k reads planes[plane_of[k]] (f32 images;
 * a 1-channel f32 upload is stored unchanged) at xyspd[4k ..] = x, y, s, pixelDistance -- and returns per job the shape u[4]
 * when the loop was left, ok and iters (the loop counter at the exit, maxIterations when the loop ran out; -1: no wavefront
 * wrote the job).  *handed_out (may be NULL): the keypoints the eight counters of variant 3 handed out, each counter clipped to
 * the length of its range (n after a complete launch; 0 for the other variants).  n = 0 returns MODSX_OK without a launch.
 * Non-finite x, y, s, pixelDistance <= 0 and planes below 4 x 4 are refused with MODSX_ERR_ARG.
 * modsx_debug_check_borders (host only): interpolateCheckBorders (detectors/helpers.cpp:524-549) as the kernels evaluate it, for n
 * tuples of 9 floats (cols, rows, ofsx, ofsy, a11, a12, a21, a22, W); touch[i] = 0 / 1.  Returns n. */
int modsx_debug_baumberg_geometry(int n, int W, int variant, int chunk, int *geometry);
int modsx_debug_baumberg_geometry_ctx(modsx_ctx *ctx, int n, int W, int variant, int chunk, int *geometry);
int modsx_debug_baumberg_variant(int W);
int modsx_debug_baumberg(modsx_ctx *ctx, const modsx_image *const *planes, int nplanes, const int *plane_of, const float *xyspd,
                         int n, const modsx_hessaff_params *par, int variant, int chunk, float *u, int *ok, int *iters,
                         int *geometry, int *handed_out);
int modsx_debug_check_borders(const float *tuples, int n, unsigned char *touch);
/* Which lane does which element in the LDS describe kernels (csrc/describe_lanes.hpp; both entries are host only).
 * modsx_debug_describe_lanes: for a window of P x P, counts[16] = blur taps, needed columns NC, rows per row tile (0: the window
 * takes the global-memory kernels), needed rows per column tile (0: global-memory kernel, -1: the sampling kernel filters the
 * columns too), then for each of sampling taps, row filter, column filter inside the sampling kernel, separate column filter
 * three lane-slot counts over the whole window: slots that hold a sample / an output pair, slots this build issues, slots the
 * rule before it issued (fixed 4-slot chunks of 4 x 64 or 8 x 32 coordinates; whole rounds of 1024 pairs), restated for comparison.
 * modsx_debug_describe_lane_map: the tap slots of one parked chunk of a row pass of `rows` (1 .. 64) rows.  rule[5] = columns of
 * a full chunk, row stride of the coordinate park (words, odd), words of the park per array, and for a chunk of nc columns
 * (1 .. the full chunk; nc = 0 asks for the first three only) the multiplier M of e / nc == e * M >> 16 and the 64-lane slots
 * issued.  map[3 e ..] = row, column, park word of sample e -- lane e % 64 of slot e / 64 -- for e < min(rows * nc, cap), computed
 * as the kernel computes them.  Returns rows * nc. */
int modsx_debug_describe_lanes(int P, long *counts);
int modsx_debug_describe_lane_map(int rows, int nc, int *rule, int *map, int cap);
/* per-stage time of the last modsx_match_pair in ms: detect, orient, describe, match, verify, total */
int modsx_last_timings(modsx_ctx *ctx, double *ms6);

/* int SetVSPars(scale_set, tilt_set, phi_base, FGINNThreshold, DistanceThreshold, descriptors, par, prev_par,
 *               InitSigma, doBlur, dsplevels, minSigma, maxSigma)            synth-detection.cpp:103-234
 * The view ladder of one step, de-duplicated against the views of earlier steps (prev[0..*nprev) is extended).
 * Returns the number of new views (host only). */
int modsx_set_vs_pars(const double *scale_set, int ns, const double *tilt_set, int nt, double phi_base,
                      double InitSigma, int doBlur, modsx_view *par, int cap, modsx_view *prev, int *nprev,
                      int cap_prev);

/* void GenerateSynthImageCorr(const cv::Mat &in_img, SynthImage &out_img, name, tilt, phi, zoom, InitSigma,
 *                             doBlur, img_id, convert2gray)                    synth-detection.cpp:236-430
 * gray: an uploaded image (gray conversion already applied).  Returns a new image handle (modsx_image_free),
 * H9 = SynthImage::H (original -> view); *is_identity = 1 when the reference takes its "original image"
 * short-cut (the handle then aliases `gray`). */
modsx_image *modsx_synth_view(modsx_ctx *ctx, const modsx_image *gray, const modsx_view *view, double *H9,
                              int *is_identity);

/* The HessianAffine / SIFT-family branch of ImageRepresentation::SynthDetectDescribeKeypoints
 * (imagerepresentation.cpp:603-2047) for the views view_begin, view_begin+view_step, ...: synthesise, detect,
 * orient, reproject to the original frame, describe.  regs: malloc'd, in view order, ids re-based as
 * AddRegions does (:588-600, :2044-2045) when the call covers all views (view_step == 1), otherwise local to
 * each view block (img_id = view index) so that shards can be merged.  desc (optional): malloc'd [n][128] f32.
 * dev_desc_u8 (optional): device buffer of capacity dev_cap regions that receives the [n][128] u8 descriptors
 * (what the matcher consumes) without leaving HBM.  view_counts (optional): [nviews] regions per view. */
int modsx_detect_describe_views(modsx_ctx *ctx, const modsx_image *img, const modsx_view *views, int nviews,
                                const modsx_pair_params *par, int view_begin, int view_step, modsx_region **regs,
                                float **desc, void *dev_desc_u8, long dev_cap, int *view_counts);

/* MatchFlannFGINN on u8 descriptors that already live in HBM (e.g. after an all-gather over xGMI) */
int modsx_match_fginn_device(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2,
                             const double *pos2, double ratio, double contradDist, int nn, modsx_tentative **out);

/* FGINN matching against a descriptor database: MatchFlannFGINNPlusDB (matching/matching.hpp:270-271, .cpp:462-572), the WxBS
 * strategy.  The squared distance dDB of a query to its nearest database descriptor is one more "second nearest": a record
 * is kept iff max(d1/d2, d1/dDB) <= ratio^2 (f32 quotients widened, std::max: a NaN d1/dDB -- the query equals its nearest train
 * AND a database row -- is ignored), its `ratio` is the square root of that maximum, and d2byDB = dDB.  With ratio >= 1 the
 * records are those of modsx_match_fginn plus d2byDB.  The search is exact (the reference asks a kd-tree).
 * modsx_db: cv::Mat descDB of mods.cpp:207-216 / CorrespondenceBank::DB, packed once into HBM: n rows of 128 values holding
 * the integers 0..255, dtype 0 = u8, 1 = f32 (anything else -- fractions, values out of range, NaN, n < 1, more than
 * MODSX_DB_MAX_ROWS rows -- gives NULL and a message).  Read-only after creation: every context of its device may use it, also
 * at the same time.  Parsing OpenCV FileStorage files is the caller's business: hand over the array. */
#define MODSX_DB_MAX_ROWS 16777216L   /* 2^24 rows (2 GiB of HBM) */
typedef struct modsx_db modsx_db;
modsx_db *modsx_db_create(modsx_ctx *ctx, const void *rows, long n, int dtype);
/* A database must outlive its attachments (modsx_set_fginn_db); freeing one that is attached to `ctx` detaches it there. */
void modsx_db_free(modsx_ctx *ctx, modsx_db *db);
long modsx_db_rows(const modsx_db *db);
/* stage tap: dmin[i] = squared L2 distance of query i ([n][128] f32 holding integers 0..255) to its nearest database row */
int modsx_db_nearest(modsx_ctx *ctx, const modsx_db *db, const float *desc, int n, float *dmin);
/* As modsx_match_fginn / modsx_match_fginn_device, plus the database (NULL, or one of another device: MODSX_ERR_ARG).
 * d2byDB (optional): malloc'd, one value per returned record (modsx_free). */
int modsx_match_fginn_db(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, const double *pos2,
                         double ratio, double contradDist, int nn, const modsx_db *db, modsx_tentative **out, double **d2byDB);
int modsx_match_fginn_db_device(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2,
                                const double *pos2, double ratio, double contradDist, int nn, const modsx_db *db,
                                modsx_tentative **out, double **d2byDB);
/* MatchPars::useDBforFGINN for the fused callers of this context (modsx_match_pair, _pairs, _pair_views, _pairs_views,
 * _ladder): every match and re-match of a class whose descriptor is MODSX_DESC_ROOT_SIFT, of either detector, goes against
 * the database, and no other class does (correspondencebank.cpp:333-341).  NULL detaches.  All contexts of one
 * modsx_match_pairs / modsx_match_pairs_views call must have the same database attached, or none (MODSX_ERR_ARG before any
 * work).  The sharded calls refuse a context with a database attached (MODSX_ERR_ARG at entry, before any collective): the
 * attachment must therefore be alike on all ranks. */
int modsx_set_fginn_db(modsx_ctx *ctx, const modsx_db *db);

/* Matching of binary descriptors (ORB, BRISK, FREAK, the AKAZE bit strings) by a distance threshold: MatchFLANNDistance
 * (matching/matching.cpp:607-666), which MatchImgReps calls for every class with DistanceThreshold > 0
 * (correspondencebank.cpp:283-284, 342-343), with binary_matcher = linear and binary_dist = HAMMING.  The search is exact (the
 * reference's default is an approximate hierarchical index).  The library does not produce such descriptors: the caller brings
 * them, e.g. a 32-value ORB class read with modsx_load_regions.
 *   descriptors  nbytes bytes per region, 1 <= nbytes <= MODSX_HAMMING_MAX_BYTES; the reference stores Row[j] = floor(desc.vec[j])
 *                as uchar.  From the host: dtype 0 = u8, dtype 1 = f32 holding the integers 0..255; anything else (fractions,
 *                values out of range, NaN, another dtype) is MODSX_ERR_ARG, the rule of every other descriptor entry.
 *   search       for every query the two nearest trains by (Hamming distance, train index) in lexicographic order: equal
 *                distances keep the lower train index, for the first neighbour and for the second.
 *   record rule  max_distance = (int)(float)distanceThreshold; a query gives a record iff d(first) <= max_distance; records come
 *                in query order: q, t0 = first, tj = t1 = second, d1 = d(first), d2 = d2by2ndcl = d(second),
 *                ratio = (double)d1 / (double)d2.  0 / 0 gives NaN and is returned as such; d1 <= d2, so no infinity occurs.
 *   edges        n1 == 0 or n2 == 0: 0 records.  n2 == 1: MODSX_ERR_ARG whatever n1 is -- the reference reads a second
 *                neighbour that was never written.  distanceThreshold <= 0 or not finite: MODSX_ERR_ARG (the reference only
 *                calls with > 0).  nbytes outside 1..64 or a side of more than 2 000 000 rows: MODSX_ERR_ARG.
 * The reference function starts with corresp.TCList.clear(): the returned records replace, they are not appended. */
#define MODSX_HAMMING_MAX_BYTES 64
/* stage tap + matcher, descriptors from the host */
int modsx_match_hamming(modsx_ctx *ctx, const void *desc1, int n1, const void *desc2, int n2, int nbytes, int dtype,
                        double distanceThreshold, modsx_tentative **out);
/* the same on dense [n][nbytes] u8 rows that already live in HBM (any alignment) */
int modsx_match_hamming_device(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2, int nbytes,
                               double distanceThreshold, modsx_tentative **out);
/* host only, no context: the record rule of matching.cpp:647-661 on the search result
 * nn2 = [n1][4] = {first, d(first), second, d(second)} -- the one copy of that rule, every entry above and below goes through it */
int modsx_hamming_tentatives(const int *nn2, int n1, double distanceThreshold, modsx_tentative **out);
/* debug: the raw search result of the device path, with the train axis forced into `splits` parts (0 = production geometry; more
 * than one per tile is cut down to one per tile); geometry[4] (optional) = {tile length in trains, splits used, workgroups of
 * k_hamming_2nn, W = ceil(nbytes / 4)}.  nn2: n1 x 4 ints, the caller's.  Needs n1 >= 1 and n2 >= 2. */
int modsx_debug_match_hamming(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2, int nbytes,
                              int splits, int *nn2, int *geometry);
/* host only, no context: the geometry modsx_debug_match_hamming would report for these sizes (one function of n1, n2, W) */
int modsx_debug_hamming_geometry(int n1, int n2, int nbytes, int splits, int *geometry);
/* One binary-descriptor step of mods.cpp:229-415 on caller-supplied regions: MatchFLANNDistance + DuplicateFiltering (key =
 * ratio, as for FGINN records) + LORANSACFiltering (H or F per par) -- what modsx_match_pair leaves, with the match stage
 * replaced.  An empty side gives the zeroed result with H = -1; n2 == 1 is MODSX_ERR_ARG before any work. */
int modsx_match_regions_hamming(modsx_ctx *ctx, const modsx_region *regs1, const void *desc1, int n1,
                                const modsx_region *regs2, const void *desc2, int n2, int nbytes, int dtype,
                                double distanceThreshold, const modsx_pair_params *par, modsx_pair_result *res);

/* FGINN matching of float descriptors of any width: MatchFlannFGINN (matching/matching.cpp:357-461) with vector_matcher = linear
 * as the reference runs it on every real-valued class -- desc.vec copied into a CV_32F matrix of desc_size columns, the linear
 * index in f32 (SURF 64, LIOP 144, MROGH 192, DAISY 200, unquantised SIFT, learned 128-D / 256-D vectors, rows of a key file read
 * with modsx_load_regions).  Every other descriptor entry keeps its rule (128 values holding the integers 0..255).
 *   rows      [n][dim] f32, dim % 4 == 0 and 4 <= dim <= MODSX_FGINN32_MAX_DIM.  The % 4 rule is the loop of the linear index as
 *             the test oracle states it; the tail loop of FLANN's L2 for other widths is not restated anywhere: refused.
 *             Values must be finite with |x| <= 1e17, so that no distance overflows (256 * (2e17)^2 < FLT_MAX); anything else is
 *             MODSX_ERR_ARG.  The host entries check on the host; the device entry checks in its pack kernel and reports
 *             through a flag word that is read with the result.
 *   limits    all refused with MODSX_ERR_ARG before any launch: more than 2 000 000 rows on a side; nn outside [2, 256] (as for
 *             modsx_match_fginn); ratio NaN; ratio * ratio >= 1 -- the "all points" branch (:397-428) is NOT built for float rows.
 *   distance  for each (query, train) one f32 chain over k = 0, 4, 8, ...: e_i = a[k+i] - b[k+i],
 *             r = r + (((e0*e0 + e1*e1) + e2*e2) + e3*e3), every operation rounded to f32, no FMA, subnormals kept.
 *   order     neighbours by (distance, train index), lexicographically: equal distances keep the lower train index.
 *   walk      with the neighbours j = 0, 1, ... of a query in that order, for j = 1 .. nn - 1:
 *               1. ratio_j = (double)(d_0 / d_j), an f32 IEEE division; 0 / 0 is NaN and passes nothing
 *               2. ratio_j <= ratio^2: one record {q, t0 = idx_0, tj = idx_j, t1 = idx_1, d1 = d_0, d2 = d_j, d2by2ndcl = d_1,
 *                  ratio = sqrt(ratio_j)}, and the walk ends
 *               3. otherwise, if the f64 squared distance between pos2[idx_0] and pos2[idx_j] exceeds contradDist^2, the walk
 *                  ends without a record
 *             It also ends without a record when the trains run out (n2 < nn).  Records come in query order.
 *   result    a pure function of the inputs: not of tile length, split count, launch order or contexts in flight.
 *   edges     n1 == 0 or n2 == 0: 0 records.
 * pos2: [n2][2] f64 on the host (x, y of the train regions), also for the device entry. */
#define MODSX_FGINN32_MAX_DIM 256
/* rows from the host */
int modsx_match_fginn_f32(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2,
                          double ratio, double contradDist, int nn, modsx_tentative **out);
/* the same on dense [n][dim] f32 rows that already live in HBM (4-byte aligned, no more) */
int modsx_match_fginn_f32_device(modsx_ctx *ctx, const void *dev_desc1, int n1, const void *dev_desc2, int n2, int dim,
                                 const double *pos2, double ratio, double contradDist, int nn, modsx_tentative **out);
/* One step of mods.cpp:229-415 on caller-supplied regions: the matcher above with ratio = par->match_ratio, par->contradDist,
 * par->nn and pos2 = reproj_kp.x, y of regs2 (as the reference takes it), then DuplicateFiltering (key = ratio) and
 * LORANSACFiltering (H or F per par) -- the pair tail of modsx_match_regions_hamming with the match stage replaced.  An empty
 * side gives the zeroed result with H = -1. */
int modsx_match_regions_f32(modsx_ctx *ctx, const modsx_region *regs1, const float *desc1, int n1, const modsx_region *regs2,
                            const float *desc2, int n2, int dim, const modsx_pair_params *par, modsx_pair_result *res);
/* debug: modsx_match_fginn_f32 (rows from the host) with the train axis forced into `splits` parts (0 = production geometry; more
 * than one per tile is cut down to one per tile) and the stage behind the first switched by stage_mask: 1 = the top-4 search
 * and the host's walk over j = 1..3, 3 = + the resolve sweep (production); a query that needs a stage that is off gives no
 * record.  Outputs, each optional, the caller's memory:
 *   top4      [n1][4] keys (f32 bit pattern of the distance << 32) | train index, ascending, all ones where there is no train
 *   stage     [n1] how the query was closed: 0 = within the four nearest, 1 = by the resolve sweep (the nearest train behind
 *             the fourth that ends the walk), 2 = by the resolve sweep's count (that train passes the ratio test, but
 *             3 + count + 1 > nn - 1: the nn run out first; no counting sweep is needed, see kernels_fginn32.hip)
 *   geometry  [6] = {tile length in trains, splits used, workgroups of k_f32_topk, kernel width DK, tiles, tiles per split}
 *   counters  [4] = {queries sent to resolve, of those closed by the count, records, validity flag word}
 *   out       the records (modsx_free)
 * Needs n1 >= 1 and n2 >= 1.  Returns the record count. */
int modsx_debug_match_fginn_f32(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2,
                                double ratio, double contradDist, int nn, int splits, int stage_mask, unsigned long long *top4,
                                unsigned char *stage, int *geometry, int *counters, modsx_tentative **out);
/* host only, no context: the geometry[6] modsx_debug_match_fginn_f32 would report for these sizes (one function of its arguments) */
int modsx_debug_fginn32_geometry(int n1, int n2, int dim, int splits, int *geometry);
/* host only, no context: dpass[i] = the smallest f32 d > 0 with (double)(d0[i] / d) <= ratio[i]^2 (f32 division), found by
 * bisection over the f32 bit patterns -- what the resolve sweep compares distances with instead of dividing; +inf when no
 * finite d passes.  d0 finite and >= 0. */
int modsx_debug_fginn32_dpass(const float *d0, const double *ratio, int n, float *dpass);

/* FGINN matching under vector_dist = L1.  MatchFlannFGINN builds its index with GenFLANNIndex(keys2, par.vector_matcher,
 * par.vector_dist, par.kd_trees) (matching/matching.cpp:388); vector_dist is a key of the [Matching] section of every config file
 * and io_mods.cpp:528-548 reads L2, L1, Hamming, Mink, Hellinger, Chi_square, KL and Max.  For CV_32F rows a default OpenCV 2.4
 * cv::flann::Index takes two of them, FLANN_DIST_L2 and FLANN_DIST_L1; these are the values of `dist` below, every other value is
 * MODSX_ERR_ARG.  Every entry above is vector_dist = L2. */
enum { MODSX_DIST_L2 = 0, MODSX_DIST_L1 = 1 };
/* The f32 entries above with the distance as an argument.  dist = MODSX_DIST_L2 runs the very kernels of the entries above and
 * returns the same bits.  dist = MODSX_DIST_L1: FLANN's L1<float> functor as the linear index calls it (no early exit), restated
 * like L2 and, like every FLANN-dependent contract here, not pinned against a real OpenCV build:
 *   distance  for each (query, train) one f32 chain over k = 0, 4, 8, ...: e_i = a[k+i] - b[k+i],
 *             r = r + (((|e0| + |e1|) + |e2|) + |e3|), every operation rounded to f32, subnormals kept.
 *   rows, limits, order, result, edges   those of modsx_match_fginn_f32: dim % 4 == 0, finite with |x| <= 1e17, nn in [2, 256],
 *             ratio * ratio >= 1 (the "all points" branch) refused before any launch.
 *   walk      UNCHANGED, including what looks like a quirk: the reference compares (double)(d_0 / d_j) with ratio^2 and records
 *             ratio = sqrt(d_0 / d_j) although L1 distances are not squares (matching.cpp:437-451).  At match_ratio 0.8 the
 *             first-to-second DISTANCE ratio that passes is therefore 0.64, not 0.8. */
int modsx_match_fginn_f32_dist(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2,
                               double ratio, double contradDist, int nn, int dist, modsx_tentative **out);
int modsx_match_fginn_f32_dist_device(modsx_ctx *ctx, const void *dev_desc1, int n1, const void *dev_desc2, int n2, int dim,
                                      const double *pos2, double ratio, double contradDist, int nn, int dist, modsx_tentative **out);
/* modsx_match_regions_f32 with the matcher above; the pair tail and modsx_pair_params are unchanged */
int modsx_match_regions_f32_dist(modsx_ctx *ctx, const modsx_region *regs1, const float *desc1, int n1, const modsx_region *regs2,
                                 const float *desc2, int n2, int dim, const modsx_pair_params *par, int dist, modsx_pair_result *res);
/* modsx_debug_match_fginn_f32 with the distance: the same optional outputs */
int modsx_debug_match_fginn_f32_dist(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim,
                                     const double *pos2, double ratio, double contradDist, int nn, int dist, int splits, int stage_mask,
                                     unsigned long long *top4, unsigned char *stage, int *geometry, int *counters,
                                     modsx_tentative **out);
/* L1 for the SIFT family: rows of 128 values that hold the integers 0..255, the domain of modsx_match_fginn, searched as bytes.
 * On that domain every |e| is an integer <= 255, every group sum <= 1020 and every running sum <= 32640, all exact in f32: the
 * integer sum of absolute differences, converted to f32, IS the chain's result, and the records are bit for bit those of
 * modsx_match_fginn_f32_dist(..., 128, ..., MODSX_DIST_L1) on the same rows.
 * desc*: [n][128] f32 holding integers 0..255; anything else is refused as modsx_match_fginn refuses it, and so are nn outside
 * [2, 256], more than 2 000 000 rows on a side, a NaN ratio and, unlike there, ratio * ratio >= 1. */
int modsx_match_fginn_l1(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, const double *pos2, double ratio,
                         double contradDist, int nn, modsx_tentative **out);
/* the same on dense [n][128] u8 rows that already live in HBM (any byte alignment), as modsx_match_fginn_device takes them */
int modsx_match_fginn_l1_device(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2,
                                const double *pos2, double ratio, double contradDist, int nn, modsx_tentative **out);
/* modsx_match_regions_f32 with the matcher above.  desc*: [n][128] f32 holding the integers 0..255 (what
 * modsx_describe_regions returns), from the host. */
int modsx_match_regions_l1(modsx_ctx *ctx, const modsx_region *regs1, const float *desc1, int n1, const modsx_region *regs2,
                           const float *desc2, int n2, const modsx_pair_params *par, modsx_pair_result *res);
/* debug: modsx_match_fginn_l1 with forced `splits` and `stage_mask` and the optional outputs of modsx_debug_match_fginn_f32;
 * geometry[3] is the row width in 32-bit words (32), geometry[2] the workgroups of k_l1_topk */
int modsx_debug_match_fginn_l1(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, const double *pos2,
                               double ratio, double contradDist, int nn, int splits, int stage_mask, unsigned long long *top4,
                               unsigned char *stage, int *geometry, int *counters, modsx_tentative **out);
/* host only, no context: the geometry[6] modsx_debug_match_fginn_l1 would report for these sizes (one function of its arguments) */
int modsx_debug_fginn_l1_geometry(int n1, int n2, int splits, int *geometry);

/* One step of mods.cpp:229-415 with a ladder of synthesised views per image (same views for both images,
 * as in iters_mods_cviu.ini). */
int modsx_match_pair_views(modsx_ctx *ctx, const modsx_image *img1, const modsx_image *img2,
                           const modsx_view *views, int nviews, const modsx_pair_params *par,
                           modsx_pair_result *res);

/* The iteration ladder of mods.cpp:229-415 (`for step < maxSteps && curr_matches < minMatches`), restricted to
 * the HessianAffine + SIFT-family class with LO-RANSAC homography verification and doBeforeRANSAC = 1
 * (config_iter_mods_cviu.ini).  Step k synthesises its views for both images, APPENDS the regions to the two
 * image representations (AddRegions, imagerepresentation.cpp:552-600), re-matches everything accumulated so far
 * (MatchImgReps clears and rebuilds the class' tentatives every step, correspondencebank.cpp:291-345) and
 * verifies; the loop ends once n_verified >= min_matches.  match_ratio of a step (FGINNThreshold of that
 * iteration's section) overrides par->match_ratio when > 0.  *steps_done = steps executed.
 * Two detector classes are kept apart as in the reference (separate_detectors): a step adds regions to, and re-matches,
 * only the class of its own detector; the other class keeps its tentatives (CorrespondenceBank, correspondencebank.cpp:
 * 180-218) and GetCorresponcesVector() concatenates HessianAffine before MSER (map order).
 *   Descriptor classes (the WxBS ladder, iters_mods_cviu_wxbs.ini:35-41,48-54,61-67).  A step may carry several descriptors.
 * The reference then keeps one region list per (detector, descriptor) -- RegionVectorMap[det][desc] -- and one tentative list
 * per (descriptor, detector), each matched separately with the FGINNThreshold of its descriptor (MatchImgReps,
 * correspondencebank.cpp:291-347).  All descriptors of a step are computed on ONE oriented region list: when any of them
 * is a Half type the dominant orientations come from DetectOrientation(..., doHalfSIFT = true, ...) (opposite histogram
 * bins folded, synth-detection.cpp:801-808) and every descriptor of the step -- RootSIFT included -- is described on that
 * list (imagerepresentation.cpp:693-706, 1259-1264, 1288-1296).  The fused callers do exactly that: one orientation pass
 * (Half-folded iff a Half type is present), one pass over the patches that emits every descriptor of the step.
 *   GetCorresponcesVector("All", "All") walks std::map<descriptor name, std::map<detector name, list>> (correspondencebank.cpp:
 * 117-179), i.e. the tentatives reach DuplicateFiltering / LO-RANSAC in the order HalfRootSIFT, HalfSIFT, RootSIFT, SIFT and,
 * inside a descriptor, HessianAffine before MSER.  Region indices of the result refer to the concatenation of the per-class
 * region lists of each image in that same order (with one descriptor class: [HessianAffine regions, MSER regions]). */
typedef struct modsx_ladder_step {
  const modsx_view *views;
  int nviews;
  double match_ratio;
  int detector;      /* MODSX_DET_HESSIAN (0) or MODSX_DET_MSER: the [HessianAffineN] / [MSERN] section this step comes from */
  /* the section's Descriptors / FGINNThreshold lists; n_desc = 0: par->n_desc / desc_types / desc_ratios (and, when those are
   * empty too, the one class {par->desc_type, match_ratio}) */
  int n_desc;
  int desc_types[MODSX_MAX_DESC];
  double desc_ratios[MODSX_MAX_DESC];
} modsx_ladder_step;
int modsx_match_ladder(modsx_ctx *ctx, const modsx_image *img1, const modsx_image *img2,
                       const modsx_ladder_step *steps, int nsteps, int min_matches, const modsx_pair_params *par,
                       modsx_pair_result *res, int *steps_done);

/* ---- stored image representations: describe once, match against many ---------------------------------------------------
 * modsx_rep is the reference's ImageRepresentation (imagerepresentation.hpp): one region list with its descriptors per
 * (detector in {MODSX_DET_HESSIAN, MODSX_DET_MSER}) x (descriptor type MODSX_DESC_*) class -- RegionVectorMap[det][desc].  It lives
 * on the device of the context that made it and owns its buffers (no context's scratch), so it outlives calls.  Besides the
 * [n][128] u8 descriptors a class keeps them in the matcher's packed train form, rebuilt whole at the end of every
 * modsx_rep_add_views / modsx_rep_append on the adding context's stream and waited for there: a match that takes the
 * representation as its train side never packs it again.
 *   A representation is changed by one thread at a time.  Otherwise it is read-only: any context of its device may match
 * against it, also at the same time (as with modsx_db).  Free it after every call that uses it has returned.
 *   The sharded calls do not take representations. */
typedef struct modsx_rep modsx_rep;
modsx_rep *modsx_rep_create(modsx_ctx *ctx);
void modsx_rep_free(modsx_ctx *ctx, modsx_rep *rep);
/* One step of SynthDetectDescribeKeypoints + AddRegions (imagerepresentation.cpp:603-2047, :552-600) for one image: what one
 * image side of a modsx_match_ladder step does.  The step's views are synthesised, detected with step->detector, oriented once
 * and described with every descriptor of the step (step->n_desc, else par's list, else par->desc_type); each of those classes
 * receives the step's regions, ids re-based onto its own list.  step->match_ratio / desc_ratios are not used.  Returns the
 * regions added to each class of the step. */
int modsx_rep_add_views(modsx_ctx *ctx, modsx_rep *rep, const modsx_image *img, const modsx_ladder_step *step,
                        const modsx_pair_params *par);
/* LoadRegions (read_pre_extracted, mods.cpp:236-241): n regions and their [n][128] descriptors from the caller, appended to one
 * class with the ids as given.  dtype 0 = u8, 1 = f32 holding the integers 0..255 (anything else -- fractions, values out of
 * range, NaN, another dtype -- is MODSX_ERR_ARG).  Returns n. */
int modsx_rep_append(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs, const void *desc, int dtype,
                     int n);
/* The regions and u8 descriptors of one class as malloc'd copies (modsx_free); either pointer may be NULL.  Returns n. */
int modsx_rep_class(modsx_ctx *ctx, const modsx_rep *rep, int detector, int desc_type, modsx_region **regs, unsigned char **desc_u8);
/* Stage tap: the MatchFlannFGINN records of one class, rep1 the queries, rep2 (pre-packed) the trains with the positions
 * reproj_kp.x, y of its regions -- what modsx_match_fginn_device returns for the same descriptors and positions. */
int modsx_rep_match_fginn(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *rep2, int detector, int desc_type, double ratio,
                          double contradDist, int nn, modsx_tentative **out);
/* CorrespondenceBank::MatchImgReps(ImgRep1, ImgRep2) (correspondencebank.cpp:291-347) + GetCorresponcesVector("All", "All") +
 * DuplicateFiltering + LORANSACFiltering (H or F per par) of rep1 against each of n partners: results[i] is what
 * modsx_match_ladder leaves for a pair whose two representations hold these classes.
 *   classes: the classes to match and to verify, each with its FGINN ratio.  n_classes == 0: every class that is non-empty in
 * rep1 or in the partner, with the ratio par gives its descriptor (desc_ratios of par's list; a descriptor par does not list,
 * or a ratio that is not positive: par->match_ratio).  Classes are concatenated in map order -- descriptor types 3, 2, 1, 0,
 * HessianAffine before MSER inside a type -- and the tentatives' indices refer to that concatenation.
 *   The contexts take groups of up to 4 partners off a shared counter; a group costs one matcher launch set per class (problems
 * with an empty side are left out), verification runs on helper threads as in modsx_match_pairs_views.  A database attached
 * to the contexts applies to the RootSIFT classes (modsx_set_fginn_db; all contexts the same database, or none).  A partner
 * without regions gives the zeroed result with H = -1 and n_regions1 set.  Returns n.
 *   Float classes (MODSX_DESC_CAFFE .. MODSX_DESC_SURF, see modsx_rep_append_f32 below) are taken in classes[] as well and are part
 * of "every class" when n_classes == 0; modsx_rep_class_rank gives the order of all classes.
 *   Binary classes (MODSX_DESC_BRISK .. MODSX_DESC_ORB, see modsx_rep_append_bin below) are taken in classes[] only.  For a binary
 * class the `ratio` field is the class's DistanceThreshold (MatchFLANNDistance), not an FGINN ratio. */
typedef struct { int detector, desc_type; double ratio; } modsx_rep_class_sel;
int modsx_match_reps(modsx_ctx *const *ctxs, int n_ctx, const modsx_rep *rep1, const modsx_rep *const *reps2, int n,
                     const modsx_rep_class_sel *classes, int n_classes, const modsx_pair_params *par, modsx_pair_result *results);
/* The loop of mods_multi.cpp:232-379: one image against n partners over the iteration ladder.  Per step the representation of
 * img1 grows ONCE and every partner's grows (the images are dealt over the contexts), the classes of the step's detector are
 * re-matched for every partner with the step's ratios -- the other classes keep their tentatives, as in modsx_match_ladder --
 * and every partner is verified.  The loop ends after the first step in which ANY partner reached min_matches verified
 * correspondences (GetAtLeastOneImageMatch, mods_multi.cpp:230-232, 365-367); all partners finish that step.  results[i] is what
 * modsx_match_ladder(img1, imgs2[i], steps, *steps_done, min_matches = infinity) returns.  Restrictions are those of
 * modsx_match_ladder.  The images must live on the device of the contexts.  Returns n. */
int modsx_match_one_to_many(modsx_ctx *const *ctxs, int n_ctx, const modsx_image *img1, const modsx_image *const *imgs2, int n,
                            const modsx_ladder_step *steps, int nsteps, int min_matches, const modsx_pair_params *par,
                            modsx_pair_result *results, int *steps_done);

/* ---- view-sharded multi-GPU path (one process per GPU, RCCL over xGMI) ------------------------------------------------
 * The reference's unit of parallelism is the synthesised view (`#pragma omp parallel for` over views,
 * imagerepresentation.cpp:612-622); views meet only in AddRegions' ordered concatenation (:2044-2045, ids re-based by
 * AddRegionsToList :588-600).  View v belongs to rank v mod world.  A modsx_comm is ONE communicator per rank; the
 * 128-byte id comes from modsx_comm_unique_id() (RCCL, bound at run time with dlopen) or modsx_comm_loopback_id() on one
 * rank and reaches the others by any side channel (MPI, torch.distributed, a file, a shared variable).
 *   Lanes.  The contexts (host thread + stream) of a rank that use the communicator at the same time are its LANES:
 * modsx_comm_set_lanes(n) once, modsx_comm_attach(comm, ctx, lane) per context, one thread per lane.  Collectives are issued
 * in strict round-robin lane order, the same sequence on every rank: lane k of every rank must make the same sharded
 * calls in the same order, and every lane the same number of them per round (modsx_comm_lane_done() takes a lane that
 * has finished out of the rotation, modsx_comm_reset_lanes() puts all of them back at a quiescent point).
 *   Errors are collective: a failure on one rank (bad view, out of memory, ...) is carried in the exchanged headers and
 * every rank returns it from the same call; no rank is left waiting.  A collective that does not complete within the
 * deadline (modsx_comm_set_timeout, env MODSX_COMM_TIMEOUT_MS, default 30000) aborts the communicator: the call and all
 * later ones on it return MODSX_ERR_TIMEOUT.
 *   The loopback transport runs `world` ranks inside ONE process on ONE device (one context + host thread per rank): the
 * all-gather is `world` device-to-device copies behind an event handshake, everything above it is the code the RCCL
 * transport runs.  It exists so that world > 1 is testable on a single GPU. */
typedef struct modsx_comm modsx_comm;
int modsx_comm_unique_id(void *id128);
int modsx_comm_loopback_id(void *id128, int world);
modsx_comm *modsx_comm_create(modsx_ctx *ctx, const void *id128, int rank, int world);
void modsx_comm_destroy(modsx_comm *comm);
int modsx_comm_set_lanes(modsx_comm *comm, int nlanes);
int modsx_comm_attach(modsx_comm *comm, modsx_ctx *ctx, int lane);
int modsx_comm_lane_done(modsx_comm *comm, int lane);
int modsx_comm_reset_lanes(modsx_comm *comm);
int modsx_comm_set_timeout(modsx_comm *comm, int milliseconds);
int modsx_comm_info(const modsx_comm *comm, int *rank, int *world, int *rccl_version, long *bytes_gathered, long *collectives);
/* out[0..n): collectives issued, bytes gathered, block-size retries, agreement collectives, lanes, loopback (0/1), dead (0/1),
 * microseconds the lanes waited for their turn to issue, bytes received in owner-only exchanges, owner-only exchanges.
 * Returns the number of statistics available. */
int modsx_comm_stats(const modsx_comm *comm, long *out, int n);
/* How modsx_match_pairs_views_sharded (owner_base >= 0) moves the rows of an image side.  MODSX_EXCHANGE_ALL_GATHER (default, the
 * north star's "all-gather of regions + descriptors"): every rank receives every row.  MODSX_EXCHANGE_OWNER: the per-item counts go
 * to every rank (an all-gather of a few KB), the rows of pair g only to the rank that matches and verifies it (ncclSend / ncclRecv
 * in one group): 1 / world of the all-gather's bytes on the wire, exact sizes (no padded blocks, no retry), one more host wait per
 * call.  Set it alike on every rank before the first sharded call: it is part of the call's contract, like the view list.  The mode
 * travels in the header, and on the loopback transport (which checks sizes) ranks set differently stop with MODSX_ERR_TIMEOUT at the
 * first exchange; over RCCL they would issue all-gathers of different byte counts, which the collective library does not define
 * (a hang that ends in the communicator's deadline, or garbage that the header check then rejects) -- the library cannot detect the
 * mismatch there before the collective.  The calls that return lists to every rank keep the all-gather. */
#define MODSX_EXCHANGE_ALL_GATHER 0
#define MODSX_EXCHANGE_OWNER 1
int modsx_comm_set_exchange(modsx_comm *comm, int mode);
/* The owner-only exchange stated on the host (what the device path derives from the gathered headers; the gloo CPU test runs ranks
 * over it): item_counts[f] = regions of item f = image * nviews + view (item f belongs to rank f mod world, its rows sit in that
 * rank's local buffer in item order), image_owner[j] = the rank that reads image j.  For `rank`:
 *   sends[k] = {peer, image, first local row, rows}: the messages it sends, in issue order (images ascending);
 *   recvs[k] = {peer, image, first row of its receive buffer, rows}: the messages it receives (images ascending, then source ranks);
 *   jobs[k]  = {first row of the receive buffer, first row of the list, rows, 0}: where the rows of each item of an owned image go
 *              (list rows count ALL items: the lists keep the all-gather's positions).
 * n[0..5) = messages sent, messages received, jobs, rows of the receive buffer, list length.  cap = capacity of each array in
 * entries (4 ints each); MODSX_ERR_CAPACITY when one is too small (n[] is still filled).  Returns MODSX_OK. */
int modsx_shard_owner_plan(const int *item_counts, int nimages, int nviews, int world, int rank, const int *image_owner, int *sends,
                           int *recvs, int *jobs, int cap, long *n);
/* Where row j of the reference's list sits in the all-gathered buffer (rank r's padded block starts at r * maxrows):
 * counts[r * nviews + v] = regions of view v on rank r (0 unless r == v mod world).  Returns the list length (host only). */
int modsx_view_block_order(const int *counts, int world, int nviews, int *src, int cap, int *maxrows_out);
/* The wire format of one exchange, stated on the host -- what the pack / ordering kernels of the sharded calls do on the device
 * (the GPU tests compare the two byte for byte; the gloo CPU tests run world 2 and 3 over these functions without a device):
 *   block = header {magic "MXSH", rc, rows, items, counts[items]} padded to 64 B, then rows of R + 128 * ndesc bytes (the region
 *           part, then the region's descriptor of every class of the step), padded to block_rows rows.
 *   row_format MODSX_SHARD_ROW_REGION: R = sizeof(modsx_region) = 200, the whole region -- the calls that return region lists
 *           (modsx_detect_describe_views_sharded, the ladder);
 *   row_format MODSX_SHARD_ROW_KP: R = 56, the doubles x, y, a11, a12, a21, a22, s of the region's reproj_kp -- all that the
 *           matcher (positions) and DuplicateFiltering / LO-RANSAC read of a region: modsx_match_pairs_views_sharded, which
 *           returns pair results only (184 B per region and descriptor class on the wire instead of 328).
 * Items = (image, view) pairs, f = image * nviews + view; item f belongs to rank f mod world.
 * _bytes: size of a block.  _pack: this rank's block (counts[f] = 0 for items of other ranks; a block that is too small keeps
 * the true row count in its header).  _unpack: the reference's list from the `world` gathered blocks -- regs_out is
 * modsx_region[cap] (ROW_REGION) or double[cap][7] (ROW_KP); returns its length, MODSX_ERR_CAPACITY (*need_rows = the largest
 * row count) when a block was too small, or the rc a rank's header carries. */
#define MODSX_SHARD_ROW_REGION 0
#define MODSX_SHARD_ROW_KP 1
long modsx_shard_block_bytes(int items, int block_rows, int ndesc, int row_format);
long modsx_shard_block_pack(const modsx_region *regs, const unsigned char *const *desc, int ndesc, int n, const int *counts, int items,
                            int rc_local, int block_rows, int row_format, void *block);
long modsx_shard_blocks_unpack(const void *blocks, int world, int items, int block_rows, int ndesc, int row_format, void *regs_out,
                               unsigned char *const *desc_out, long cap, int *item_counts, int *need_rows);
/* test hooks (need a device): the same two steps through the device kernels, outputs copied back to the host */
long modsx_shard_device_pack(modsx_ctx *ctx, const modsx_region *regs, const unsigned char *const *desc, int ndesc, int n, int row_format,
                             void *rows_out);
long modsx_shard_device_unpack(modsx_ctx *ctx, const void *blocks, int world, int items, int block_rows, int ndesc, int row_format,
                               void *regs_out, unsigned char *const *desc_out, double *pos_out, long cap);
/* SynthDetectDescribeKeypoints with this rank taking views rank, rank + world, ...: one all-gather of padded blocks
 * (header with the per-view counts + rows of modsx_region + 128 u8 descriptor bytes = 328 B), device to device; the
 * reference's order is rebuilt on the device from the gathered headers; every rank returns
 * ALL regions in reference order with re-based ids.  *dev_desc_u8 = the [n][128] u8 descriptors in HBM (owned by ctx,
 * valid until its next sharded call). */
int modsx_detect_describe_views_sharded(modsx_ctx *ctx, modsx_comm *comm, const modsx_image *img, const modsx_view *views,
                                        int nviews, const modsx_pair_params *par, modsx_region **regs, void **dev_desc_u8,
                                        int *view_counts);
/* MatchFlannFGINN with the query rows split over the ranks (every rank holds all descriptors of both images): the
 * per-query result rows are all-gathered on the device, every rank returns the full tentative list in query order. */
int modsx_match_fginn_sharded(modsx_ctx *ctx, modsx_comm *comm, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8,
                              int n2, const double *pos2, double ratio, double contradDist, int nn, modsx_tentative **out);
/* modsx_match_pair_views over the ranks: both images sharded by view, the match sharded by query row, DuplicateFiltering +
 * LO-RANSAC on rank `owner` only (owner < 0: on every rank); the other ranks fill the counters up to n_tentatives. */
int modsx_match_pair_views_sharded(modsx_ctx *ctx, modsx_comm *comm, const modsx_image *img1, const modsx_image *img2,
                                   const modsx_view *views, int nviews, const modsx_pair_params *par, int owner,
                                   modsx_pair_result *res);
/* n_pairs (1..16) multi-view pairs in ONE sharded call -- what keeps the fixed costs of the exchange from growing with the world
 * size: the views of all 2 n_pairs images form one item list (item f = image * nviews + view belongs to rank f mod world), so a
 * rank's launch sets hold ~2 n_pairs nviews / world views whatever the world size; ONE all-gather moves the rows of every image
 * side (MODSX_SHARD_ROW_KP: 56 B of geometry + the u8 descriptors of a region).  owner_base >= 0: pair g is matched AND verified by rank (owner_base + g) mod world -- the
 * exchange left all it needs there -- so the call holds ONE collective; results[g] is what modsx_match_pair_views returns for
 * pair g on that rank, the other ranks fill n_regions1 / n_regions2 only.  owner_base < 0: every rank returns every pair (the
 * query rows of the n_pairs problems of a descriptor class are split over the ranks, ONE all-gather of result rows per class).
 * A rank that fails after the exchange (out of memory in its own matcher) returns the error alone; its peers meet the
 * communicator's deadline at their next collective, as for a rank that died.  Returns n_pairs. */
int modsx_match_pairs_views_sharded(modsx_ctx *ctx, modsx_comm *comm, const modsx_image *const *imgs1, const modsx_image *const *imgs2,
                                    int n_pairs, const modsx_view *views, int nviews, const modsx_pair_params *par, int owner_base,
                                    modsx_pair_result *results);
/* modsx_match_ladder over the ranks (configs[3]: the iteration ladder with every step's views sharded): each step's
 * regions are exchanged and appended to the accumulated lists on every rank, the match is sharded by query row, and every
 * rank runs DuplicateFiltering + LO-RANSAC on the same tentatives with the same seed; the verified count that decides the
 * min_matches exit is all-gathered (4 bytes per rank and step) and the call fails on every rank (MODSX_ERR_INTERNAL) should
 * the ranks ever disagree, so no rank can leave the loop alone.  Results are identical on every rank and equal to
 * modsx_match_ladder's. */
int modsx_match_ladder_sharded(modsx_ctx *ctx, modsx_comm *comm, const modsx_image *img1, const modsx_image *img2,
                               const modsx_ladder_step *steps, int nsteps, int min_matches, const modsx_pair_params *par,
                               modsx_pair_result *res, int *steps_done);

/* Key files: void ImageRepresentation::SaveRegions(std::string fname, int mode) / LoadRegions(std::string fname)
 * (imagerepresentation.cpp:2139-2215; mods.cpp:236-241 reads them instead of detecting when read_pre_extracted is
 * set).  Text format, one (detector, descriptor) class after the other; files are byte-identical to the reference's
 * for the same lists.  A class = the AffineRegionVector of RegionVectorMap[det_name][desc_name]: n regions, their
 * descriptors as n rows of `stride` floats of which the first `dim` are written. */
typedef struct modsx_region_class {
  const char *det_name, *desc_name;
  const modsx_region *regs;
  const float *desc;
  int n, dim, stride;
} modsx_region_class;
int modsx_save_regions(const char *path, const modsx_region_class *classes, int nclasses);
/* Loads the class (det_name, desc_name) -- NULL / "" = the first class in the file.  regs and desc ([n][*dim]) are
 * malloc'd (modsx_free); found_det / found_desc (optional, >= 64 bytes) receive the names.  Returns n. */
int modsx_load_regions(const char *path, const char *det_name, const char *desc_name, modsx_region **regs, float **desc,
                       int *dim, char *found_det, char *found_desc);

/* ---- Normalised patches and the LIOP descriptor -----------------------------------------------------------------------------
 * DescribeRegions<FuncType> (synth-detection.hpp:169-255, called for LIOP at imagerepresentation.cpp:1615-1623) cuts a window
 * of mrSize * s around every region, blurs it, resamples it to patchSize x patchSize, runs photometricallyNormalize
 * (detectors/helpers.cpp:666-715) and hands the patch to the functor.  For SIFTDescriptor that is modsx_describe_regions; the
 * entries below expose the patch itself and the LIOP functor.  patchSize must be 41, as everywhere in this library; mrSize,
 * fast_extraction and photoNorm mean what they mean for modsx_describe_regions.  LIOP has no parameters: LIOPDescriptor builds
 * vl_liopdesc_new_basic(patchSize) (matching/liopdesc.hpp:55-63: 4 neighbours, 6 spatial bins, radius 6, intensity threshold
 * -(5 / 255)); the neighbours / bins / radius / threshold keys of a [LIOPDescriptor] section never reach VLFeat.
 * Every entry: n < 0, patchSize != 41 or a null pointer is MODSX_ERR_ARG (nothing is launched); n == 0 succeeds and writes
 * nothing.  The _device forms take a DEVICE pointer for the output (and, for modsx_liop_patches_device, the input), 4-byte
 * aligned, dense rows; they return after the work has finished.  The entries that compute return n. */
#define MODSX_LIOP_DIM 144
#define MODSX_LIOP_PIXELS 673
/* the patches DescribeRegions<> hands to its functor (synth-detection.hpp:214-238): patches [n][41][41] f32 */
int modsx_extract_patches(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize,
                          int fast_extraction, int photoNorm, float *patches);
int modsx_extract_patches_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                 int patchSize, int fast_extraction, int photoNorm, void *dev_patches);
/* vl_liopdesc_process (vlfeat/vl/liop.c:440-555) on n patches [n][41][41] f32 -> desc [n][144] f32, bit for bit what the
 * reference's code gives, the order of equal intensities in its patch_sort (vl/qsort-def.h:126-165) included: the spatial bins
 * are cut by rank, so that order decides the bin of pixels that tie across a cut.  Patch values must be finite (the reference's
 * comparator, an f32 difference tested <= 0, is inconsistent on NaN and infinities: such rows give unspecified descriptors, no
 * fault); -0 ties with +0; subnormal values are compared, not flushed.  The two samples of liop.c:513-516 that touch column /
 * row 41 (pixels (34, 20) and (20, 34), weights exactly 0) read nothing outside the patch: what lies outside its 1681 floats
 * counts as 0.0. */
int modsx_liop_patches(modsx_ctx *ctx, const float *patches, int n, int patchSize, float *desc);
int modsx_liop_patches_device(modsx_ctx *ctx, const void *dev_patches, int n, int patchSize, void *dev_desc);
/* DescribeRegions<LIOPDescriptor>(regions, image, liop, mrSize, patchSize, fast_extraction, photoNorm)
 * (imagerepresentation.cpp:1615-1623): desc [n][144] f32 = modsx_liop_patches of modsx_extract_patches.  The patches stay on
 * the device, in a per-context buffer of at most 64 MiB that the call fills and consumes in sub-batches. */
int modsx_describe_regions_liop(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                int patchSize, int fast_extraction, int photoNorm, float *desc);
int modsx_describe_regions_liop_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                       int patchSize, int fast_extraction, int photoNorm, void *dev_desc);
/* host only: the tables of vl_liopdesc_new_basic(patchSize) (liop.c:346-395) -- pixels[i] = x + 41 y of measurement pixel i
 * (raster order), sx / sy [i][4] = neighSamplesX / Y, built with libm as the reference builds them.  Fills the first `cap`
 * pixels (any of the three pointers may be NULL) and returns their number, 673. */
int modsx_liop_tables(int patchSize, int *pixels, double *sx, double *sy, int cap);
/* debug: modsx_liop_patches (patches from the host) that also reports, per patch, path[i] = 0 when no group of equal
 * intensities lay across a bin cut (any order by key is the reference's; perm is the stable one) or 1 when one did (perm is the
 * reference's patch_sort permutation, replayed), and perm [n][673] = measurement pixel of every rank */
int modsx_debug_liop(modsx_ctx *ctx, const float *patches, int n, int patchSize, float *desc, int *path, int *perm);
/* LIOP work of this context since modsx_create, cumulative (measurement hook): calls that launched, patches described, patches
 * that took the exact path, sub-batches (launches of the LIOP kernel).  Fills out[0 .. min(n, 4) - 1], returns 4. */
int modsx_liop_counters(modsx_ctx *ctx, long *out, int n);

/* ---- DSP-SIFT: pooled raw SIFT histograms and the f32 SIFT norm --------------------------------------------------------------
 * The "DSPSIFT" branch of the reference (domain-size pooling, imagerepresentation.cpp:1547-1598) describes every region at
 * numScales + 1 measurement sizes with SIFTDescriptor{useRootSIFT = false, doNorm = false}, adds the raw 128-bin histograms in
 * f32 in scale order, and applies SIFTnorm(std::vector<float>&) (matching/siftdesc.cpp:263-278) -- the f32 overload, not the f64
 * norm behind modsx_describe_regions.  The result is a row of 128 integers 0..255 held in f32, which the int8 matcher
 * (modsx_match_fginn), modsx_match_regions_f32, the key file and modsx_rep_append take as they are.  The entries below give the two halves and the whole.
 * DSP-SIFT is no descriptor class of modsx_describe_regions (desc_type stays 0..3), of the ladder, of modsx_rep or of the
 * sharded path.  patchSize must be 41; mrSize, fast_extraction and photoNorm mean what they mean for modsx_describe_regions.
 * Every entry: n < 0, patchSize != 41, a null pointer, a measurement size that is not finite and positive, or a region whose
 * window modsx_describe_regions would refuse (a blur of more than 512 taps) is MODSX_ERR_ARG with a message, before anything is
 * launched; n == 0 succeeds and writes nothing.  The _device forms take DEVICE pointers, 4-byte aligned, dense rows; they
 * return after the work has finished.  The entries that compute return n. */
/* the output of the doNorm = false functor (siftdesc.cpp:436-440): hist [n][128] f32 = (float) of samplePatch's f64 bins */
int modsx_describe_regions_raw(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize,
                               int fast_extraction, int photoNorm, float *hist);
int modsx_describe_regions_raw_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                      int patchSize, int fast_extraction, int photoNorm, void *dev_hist);
/* SIFTnorm(std::vector<float>&) with par.maxBinValue = maxBinValue on rows [n][128] f32 -> out [n][128] f32 holding 0..255, bit
 * for bit: the length is a serial f32 sum of the 32 group sums ((v0^2 + v1^2) + v2^2) + v3^2, its square root f32, the factor
 * (float)(1.0 / (double)len); values above maxBinValue (compared in f64) become (float)maxBinValue and the row is normalised
 * again; b = (int)((double)(512.0f * v) + 0.5) clamped to 0..255.  For callers that pool histograms of their own.  out may be
 * rows.  Rows must be finite: a row of zeros gives zeros (as the reference does on x86-64, where its NaN values convert to
 * INT_MIN); NaN and infinities give unspecified values, no fault. */
int modsx_sift_norm_rows(modsx_ctx *ctx, const float *rows, int n, double maxBinValue, float *out);
int modsx_sift_norm_rows_device(modsx_ctx *ctx, const void *dev_rows, int n, double maxBinValue, void *dev_out);
/* the whole branch: pass k = 0 .. numScales at mrSize_k = mrSize * (startCoef + k * (endCoef - startCoef) / numScales), evaluated
 * in f64 as written, pooled in f32 in that order, then the norm: desc [n][128] f32 holding 0..255.  numScales outside 1..64 is
 * MODSX_ERR_ARG (the reference divides by zero at 0), and so is any mrSize_k that is not finite and positive; all scales are
 * checked before the first runs. */
int modsx_describe_regions_dspsift(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                   int patchSize, int fast_extraction, int photoNorm, int numScales, double startCoef, double endCoef,
                                   double maxBinValue, float *desc);
int modsx_describe_regions_dspsift_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                          int patchSize, int fast_extraction, int photoNorm, int numScales, double startCoef,
                                          double endCoef, double maxBinValue, void *dev_desc);
/* DSP-SIFT work of this context since modsx_create, cumulative (measurement hook): modsx_describe_regions_dspsift calls that
 * launched, regions described, scale passes launched.  Fills out[0 .. min(n, 3) - 1], returns 3. */
int modsx_dsp_counters(modsx_ctx *ctx, long *out, int n);

/* ---- The SURF descriptor (OpenSURF U-SURF-64 on normalised patches) ----------------------------------------------------------
 * The "SURF" branch of the reference (imagerepresentation.cpp:1829-1838) runs DescribeRegions<SURFDescriptor>: the same window
 * -> blur -> 41 x 41 resample -> photometricallyNormalize front end as LIOP (modsx_extract_patches), then a functor
 * (descriptors/surfdescriptor.hpp:13-37) that builds OpenSURF's integral image of the patch / 255 and describes ONE fixed,
 * upright interest point at x = y = patchSize / 2.0f of scale (float)(patchSize / mrSize) with Surf::getDescriptor(true)
 * (opensurf/surf.cpp:152-248): 4 x 4 sub-regions x (dx, dy, |dx|, |dy|), 64 f32.  mrSize is therefore used twice, for the
 * measurement window and for the scale; the fields thres, octaves, intervals and init_sample of SURFParams never reach the
 * functor.  Results are bit for bit the reference's: the order of its f32 adds (row sums, then column sums of the integral image;
 * the 81 samples of a sub-region; the 16 length terms) and its f64 normalisation are kept; the gaussian weights come from the C
 * library's expf on the host, as the reference's do.  At the default mrSize 5.1962 the scale is 7.89, most samples lie outside
 * the patch and 28 of the 64 entries are identically zero.  A patch whose responses are all zero (a patch of zeros, or any patch
 * when the rounded scale is 0, mrSize > 82) has length 0 and gives a row of 64 NaN, as the reference does; sign and payload of
 * those NaN are unspecified.  Patch values must be finite.
 * SURF is no descriptor class of modsx_describe_regions (desc_type stays 0..3), of the ladder or of the sharded path; the rows
 * go to modsx_match_regions_f32 at dim 64 or into a stored representation (modsx_rep_describe_append), finite rows only.  The detector (FastHessian) and getOrientation are
 * not part of this library.
 * Every entry: n < 0, patchSize != 41, a null pointer, an mrSize that is not finite and positive, or an mrSize below
 * patchSize / 1024 (scale above 1024: beyond it the reference's int sample coordinates and the int squares inside its gaussian
 * approach overflow) is MODSX_ERR_ARG with a message, before anything is launched; n == 0 succeeds and writes nothing.  The
 * _device forms take DEVICE pointers, 4-byte aligned, dense rows; they return after the work has finished.  The entries that
 * compute return n. */
#define MODSX_SURF_DIM 64
/* the functor on n patches [n][41][41] f32 -> desc [n][64] f32 */
int modsx_surf_patches(modsx_ctx *ctx, const float *patches, int n, int patchSize, double mrSize, float *desc);
int modsx_surf_patches_device(modsx_ctx *ctx, const void *dev_patches, int n, int patchSize, double mrSize, void *dev_desc);
/* DescribeRegions<SURFDescriptor>(regions, image, surf, mrSize, patchSize, fast_extraction, photoNorm): desc [n][64] f32 =
 * modsx_surf_patches of modsx_extract_patches.  The patches stay on the device, in the per-context buffer of at most 64 MiB
 * that modsx_describe_regions_liop uses, filled and consumed in sub-batches. */
int modsx_describe_regions_surf(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                int patchSize, int fast_extraction, int photoNorm, float *desc);
int modsx_describe_regions_surf_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                       int patchSize, int fast_extraction, int photoNorm, void *dev_desc);
/* host only: the constants of (patchSize, mrSize) the kernel reads -- sample_x24[k + 12] for k = -12 .. 11 and sample_y24[l + 12]
 * for l = -12 .. 11 (the sample coordinates, which depend on k resp. l alone for an upright point), w1 [16][81] = gauss_s1 of
 * sub-region q = 4 (i index) + (j index) and sample 9 (k - i) + (l - j), w2 [16] = gauss_s2, *haar_size = 2 * fRound(scale).
 * Any pointer may be NULL.  Returns 0, or MODSX_ERR_ARG as above. */
int modsx_surf_tables(int patchSize, double mrSize, int *sample_x24, int *sample_y24, float *w1, float *w2, int *haar_size);
/* SURF work of this context since modsx_create, cumulative (measurement hook): calls that launched, patches described,
 * sub-batches (launches of the SURF kernel).  Fills out[0 .. min(n, 3) - 1], returns 3. */
int modsx_surf_counters(modsx_ctx *ctx, long *out, int n);

/* ---- The DAISY descriptor (libdaisy on normalised patches) ----------------------------------------------------------------------
 * The "DAISY" branch of the reference (imagerepresentation.cpp:1954-1963) runs DescribeRegions<DAISYDescriptor>: the same window
 * -> blur -> 41 x 41 resample -> photometricallyNormalize front end as LIOP and SURF (modsx_extract_patches), then a functor
 * (descriptors/daisydescriptor.hpp:33-92) that converts the patch to bytes (round half to even, saturated), hands it to libdaisy
 * and reads the descriptor of ONE fixed point at x = y = patchSize / 2, orientation 0: histq = 8 gradient-direction layers of the
 * blurred patch / 255, smoothed into radq cubes of growing sigma, sampled bilinearly at the centre and at radq rings of thq grid
 * points up to radius rad, (radq * thq + 1) * 8 f32 (200 at the reference's defaults rad 15, radq 3, thq 8, histq 8), then
 * normalised: nrm_type 0 = NRM_PARTIAL (each 8-bin histogram by its own l2 norm; a histogram of norm 0 stays 0), 1 = NRM_FULL
 * (the whole row), 2 = NRM_SIFT (up to 5 rounds of: divide by the norm if it exceeds 1e-5, clip at 0.154f; until nothing clips).
 * mrSize only sizes the measurement window; the DAISY point and its grid do not depend on it.  Results are bit for bit the
 * reference's: every f32 multiply and add of its filters (rows, then columns, taps in order, borders replicated), of the bilinear
 * mix and of the norms keeps its order; taps, layer directions, grid points and weights come from the C library's expf, cos and
 * sin on the host, as the reference's do.  A grid point outside [0, 40) on either axis, or one whose integer part is 39 or more,
 * gives 8 zeros: at rad = 20, radq = 3, thq = 8 those are histograms 17 and 19.  A patch without gradients gives a row of zeros.
 * Rows of patches with non-finite values are unspecified.
 * DAISY is no descriptor class of modsx_describe_regions (desc_type stays 0..3), of the ladder or of the sharded path; the rows
 * go to modsx_match_regions_f32 at their width or into a stored representation (modsx_rep_describe_append).
 * Accepted: patchSize == 41, histq == 8, 1 <= thq <= 8, 1 <= radq <= 3, 1 <= rad <= 20 (no grid point then leaves [0, 40]),
 * nrm_type 0 .. 2.  Every entry: anything else, n < 0 or a null pointer is MODSX_ERR_ARG with a message, before anything is
 * launched, and the context stays usable; n == 0 succeeds and writes nothing.  The _device forms take DEVICE pointers, 4-byte
 * aligned, dense rows; they return after the work has finished.  The entries that compute return n. */
#define MODSX_DAISY_MAX_DIM 200
#define MODSX_DAISY_MAX_TAPS 51
/* host only: (radq * thq + 1) * histq, or MODSX_ERR_ARG for values outside the accepted ranges */
int modsx_daisy_dim(int radq, int thq, int histq);
/* the functor on n patches [n][41][41] f32 -> desc [n][modsx_daisy_dim] f32 */
int modsx_daisy_patches(modsx_ctx *ctx, const float *patches, int n, int patchSize, int rad, int radq, int thq, int histq, int nrm_type,
                        float *desc);
int modsx_daisy_patches_device(modsx_ctx *ctx, const void *dev_patches, int n, int patchSize, int rad, int radq, int thq, int histq,
                               int nrm_type, void *dev_desc);
/* DescribeRegions<DAISYDescriptor>(regions, image, daisy, mrSize, patchSize, fast_extraction, photoNorm): desc [n][dim] f32 =
 * modsx_daisy_patches of modsx_extract_patches.  The patches stay on the device, in the per-context buffer of at most 64 MiB
 * that modsx_describe_regions_liop uses, filled and consumed in sub-batches (MODSX_DAISY_BATCH patches each, read once per
 * process; default: what fits the buffer). */
int modsx_describe_regions_daisy(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize,
                                 int fast_extraction, int photoNorm, int rad, int radq, int thq, int histq, int nrm_type, float *desc);
int modsx_describe_regions_daisy_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                        int patchSize, int fast_extraction, int photoNorm, int rad, int radq, int thq, int histq,
                                        int nrm_type, void *dev_desc);
/* host only: the constants of (rad, radq, thq, histq) the kernel reads -- k5 [5] the gaussian of sigma 0.5; kos8 / zin8 [8] the
 * layer directions; fsz [1 + radq] and taps [1 + radq][MODSX_DAISY_MAX_TAPS] (zero beyond fsz) the filters, 0: the smoothing of
 * the layers, 1 + r: the step to cube r; selected [radq] the cube of ring r; and per grid point g (0: the centre, 1 + r thq + t
 * the others) state [npts] (0 skipped, 1 zeroed, 2 sampled), base [npts] (pixel A = 41 y + x) and w [npts][4] (w0 .. w3, applied
 * to A, C = A + 1, B = A + 41, D = A + 42 in this order).  Any pointer may be NULL.  Returns 0, or MODSX_ERR_ARG as above. */
int modsx_daisy_tables(int rad, int radq, int thq, int histq, float *k5, float *kos8, float *zin8, int *fsz, float *taps, int *selected,
                       int *state, int *base, float *w);
/* DAISY work of this context since modsx_create, cumulative (measurement hook): calls that launched, patches described,
 * sub-batches (launches of the DAISY kernel).  Fills out[0 .. min(n, 3) - 1], returns 3. */
int modsx_daisy_counters(modsx_ctx *ctx, long *out, int n);

/* ---- The SURF detector (OpenSURF FastHessian) ------------------------------------------------------------------------------
 * The "SURF" detector branch of the reference (imagerepresentation.cpp:1046-1076): Integral() of the view / 255, then
 * FastHessian(int_img, ipts, octaves, intervals, init_sample, thres).getIpoints() (opensurf/fasthessian.cpp, integral.cpp,
 * integral.h, responselayer.h), bit for bit: the integral image with the reference's order of f32 adds, 4 + 2 (octaves - 1) box
 * filter response layers (filters 9, 15, 21, 27 | 39, 51 | 75, 99 | 147, 195 | 291, 387), the 3 x 3 x 3 extremum test across layers
 * of different density (read through the integer quotient of the layer WIDTHS, as getResponse does) and the sub-pixel step in
 * f64.  Points come out in the reference's push order: octave, interval, raster position of the sparsest layer.
 *   inverse   interpolateStep calls cvInvert(H, H_inv, CV_SVD); here the 3 x 3 inverse is the closed-form adjugate over the
 *             determinant in f64 with a fixed order of operations, all zeros where the determinant is 0 or not finite (the point
 *             then stays at its grid position).  This is the one step whose parity with a real OpenCV is not pinned.
 *   params    normalised as FastHessian::saveParameters does: octaves outside 1..4 give 5, intervals outside 1..4 give 4 (nothing
 *             reads it afterwards), init_sample outside 1..6 gives 2, thresh < 0 (or NaN) gives 0.0004f.
 *   refusals  MODSX_ERR_ARG with a message, before any launch: a null pointer, n_imgs < 0, an image for which a layer the
 *             parameters ask for has width or height 0 (cols / init_sample / 2^(octaves - 1) == 0, or rows likewise: the
 *             reference's assert aborts there).  n_imgs == 0 succeeds.  Pixels must be finite.
 * No orientation is assigned (the branch calls no getOrientation): keypoints carry the frame of orientation 0.  SURF is no
 * detector of the ladder, of modsx_rep_add_views or of the sharded path; a stored representation has float classes for it. */
#define MODSX_DET_SURF 6                 /* detector_type DET_SURF, detectors/structures.hpp */
#define MODSX_SURFDET_MAX_LAYERS 12
typedef struct modsx_surfdet_params {
  int octaves, intervals, init_sample;   /* the [SURF] section of the config files: 4, 4, 2 */
  float thresh;                          /* 0.0004 */
} modsx_surfdet_params;
/* out: malloc'd (modsx_free) keypoints as the branch fills det_kp: x, y, s = the Ipoint's f32 x, y, scale widened to double,
 * a11 = cos(0.0), a12 = sin(0.0), a21 = -sin(0.0) (that is -0.0), a22 = cos(0.0), every other field 0.  Returns their number. */
int modsx_detect_surf(modsx_ctx *ctx, const modsx_image *img, const modsx_surfdet_params *par, modsx_keypoint **out);
/* The same for n_imgs images of any sizes with shared launches: out = the keypoints of image 0, then image 1, ...;
 * counts[i] = the number of image i.  Returns the total.  Each image's list equals what modsx_detect_surf gives for it. */
int modsx_detect_surf_batch(modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_surfdet_params *par,
                            modsx_keypoint **out, int *counts);
/* host only: regions of SURF keypoints as the branch leaves them -- type = MODSX_DET_SURF, det_kp as given (no scaling and no
 * rectification: the branch does none), img_id, id = index, the rest as modsx_detect_affine_regions leaves it.  Returns n. */
int modsx_surf_regions(const modsx_keypoint *kps, int n, int img_id, modsx_region *out);
/* host only: the layer table the kernels would build for a rows x cols image, layers [MODSX_SURFDET_MAX_LAYERS][4] = (width,
 * height, step, filter) (may be NULL).  Returns the number of layers, or MODSX_ERR_ARG as above. */
int modsx_surfdet_geometry(int rows, int cols, const modsx_surfdet_params *par, int *layers);
/* host only: *out = the parameters as saveParameters stores them */
int modsx_surfdet_normalise(const modsx_surfdet_params *par, modsx_surfdet_params *out);
/* Stage tap of one image.  integral [rows][cols]; layers as modsx_surfdet_geometry; resp (f32) / lap (u8): every plane, one after
 * the other in layer order; the raw extrema in push order, the first cap_ext of them: ext [cap_ext][4] = (octave, interval, r, c
 * of the t layer), dD [.][3] = (dx, dy, ds), H [.][6] = (dxx, dxy, dxs, dyy, dys, dss), x [.][3] = (xc, xr, xi), accepted [.],
 * laplacian [.]; *n_ext = how many there are (call again with a larger cap_ext when it exceeds cap_ext).  Returns the number of
 * layers. */
int modsx_debug_surfdet(modsx_ctx *ctx, const modsx_image *img, const modsx_surfdet_params *par, float *integral, int *layers, float *resp,
                        unsigned char *lap, int *ext, double *dD, double *H, double *x, int *accepted, int *laplacian, int cap_ext,
                        int *n_ext);
/* SURF detector work of this context since modsx_create, cumulative (measurement hook): calls that launched, images, extrema
 * found, points accepted, regrows of the point buffer.  Fills out[0 .. min(n, 5) - 1], returns 5. */
int modsx_surfdet_counters(modsx_ctx *ctx, long *out, int n);

/* ---- The KAZE detector (AKAZE nonlinear scale space, Hessian extrema) -----------------------------------------------------
 * The "KAZE" detector branch of the reference (imagerepresentation.cpp:678-681, 1132-1152): aka::AKAZE::
 * Create_Nonlinear_Scale_Space and Feature_Detection (akaze/src/lib/AKAZE.cpp, nldiffusion_functions.cpp, fed.cpp) on the view
 * / 255, bit for bit with what those three sources compute when compiled unmodified against tools/kaze_standin/, the one place
 * where the arithmetic of the OpenCV calls they make is specified.  None of these rules is pinned against a real OpenCV:
 *   input         pixels * 1.0 / 255.0 is each f32 pixel times (float)(1.0 / 255.0).
 *   GaussianBlur  (f32, BORDER_REPLICATE) the library's gaussian_kernel(n, sigma) and two-pass order (modsx_gaussian_blur's), with
 *                 AKAZE's size rule ceil(2 (1 + (sigma - 0.8) / 0.3)) made odd: 9 taps at sigma 1.6, 5 at sigma 1.
 *   Scharr / sepFilter2D   f32, BORDER_REFLECT_101: a row pass into an f32 plane, then a column pass; taps in ascending index
 *                 order, every product and every add rounded to f32, starting from the first product.  Kernels [-1, 0, 1] and
 *                 [3, 10, 3] for Scharr, those of compute_derivative_kernels otherwise.  The kernels read only the three non-zero
 *                 taps: a zero tap adds +-0, and -0 and +0 are not told apart anywhere downstream.
 *   Mat expressions  element-wise f32 operations, each rounded: X / (k*k) is X * (float)(1.0 / (double)(k*k)), 1.0 + X an f32 add,
 *                 1.0 / X an IEEE f32 division, L * n a multiply by (float)n, Ld + Lstep an f32 add.
 *   resize        (INTER_AREA) (((a + b) + c) + d) * 0.25f with a, b the upper row where both ratios are exactly 2; otherwise the
 *                 area table: per axis, scale = ssize / (double)dsize, fs1 = d * scale, fs2 = fs1 + scale, cell = min(scale, ssize -
 *                 fs1), s2 = min(floor(fs2), ssize - 1), s1 = min(ceil(fs1), s2); a leading entry (s1 - 1, (float)((s1 - fs1) /
 *                 cell)) if s1 - fs1 > 1e-3, entries (s, (float)(1.0 / cell)) for s1 <= s < s2, a trailing entry (s2,
 *                 (float)(min(min(fs2 - s2, 1.0), cell) / cell)) if fs2 - s2 > 1e-3; per source row buf[dx] += S[sx] * alpha in
 *                 table order in f32 from 0; per destination row sum = beta * buf for the first source row, sum += beta * buf after.
 *   cv::solve     (2 x 2, DECOMP_LU) d = (double)a00 * a11 - (double)a01 * a10; if d != 0: x0 = (float)(((double)b0 * a11 -
 *                 (double)b1 * a01) * (1 / d)), x1 = (float)(((double)b1 * a00 - (double)b0 * a10) * (1 / d)); if d == 0 the offsets
 *                 keep what they held: zeros at first, the previous point's afterwards (the reference declares dst outside its loop).
 * Everything else is the reference's own code, pinned by tests/golden/kaze_ref.npz: the level table and fed_tau_by_process_time with
 * reordering, compute_k_percentile (its float counters as min(count, 2^24)), pm_g2, nld_step_scalar (0.5 * stepsize * (f32 sum) is
 * an f64 product rounded on store; the corners of Lstep stay 0), Compute_Multiscale_Derivatives, Ldet = lxx * lyy - lxy * lxy
 * without FMA, Find_Scale_Space_Extrema and Do_Subpixel_Refinement.  The 3 x 3 maxima are compacted on the device in (level, raster)
 * order; the two filter passes and the refinement's erase loop are order-dependent and run on the host as written.
 *   refusals  MODSX_ERR_ARG with a message, before any launch: a null pointer, n_imgs < 0, an image under 3 x 3, omax outside
 *             1 .. 8, nsublevels < 1, more than MODSX_KAZE_MAX_LEVELS levels, soffset or derivative_factor not positive, a
 *             derivative distance outside 1 .. 8 or more than MODSX_KAZE_MAX_TAU diffusion steps in a level (the defaults give 2 ..
 *             4 and at most 14), kcontrast_nbins outside 1 .. 4096, descriptor outside 0 .. 5, and a diffusivity other than
 *             PM_G2 (1): PM_G1, WEICKERT and CHARBONNIER call exp / pow / sqrt of OpenCV, whose arithmetic is not specified here.
 *             n_imgs == 0 succeeds.  Pixels must be finite.  A flat image has k = 0: its planes hold NaN and it has no keypoint.
 * No orientation is assigned (the branch calls no Compute_Main_Orientation) and no AKAZE descriptor (M-LDB, M-SURF) is computed.
 * KAZE is no detector of the ladder, of modsx_rep_add_views, of stored representations or of the sharded path. */
#define MODSX_DET_KAZE 9                 /* detector_type DET_KAZE, detectors/structures.hpp */
#define MODSX_KAZE_MAX_LEVELS 32
#define MODSX_KAZE_MAX_TAU 64
typedef struct modsx_kaze_params {
  int omax, nsublevels;                        /* AKAZEOptions: 4, 4 */
  float soffset, derivative_factor;            /* 1.6, 1.5 */
  float dthreshold, min_dthreshold;            /* 0.001, 0.00001 */
  float kcontrast_percentile;                  /* 0.7 */
  int kcontrast_nbins;                         /* 300 */
  int descriptor;                              /* 5 (MLDB): only its class matters, smax = 10 sqrt(2) for 0, 1, 4, 5 and 12 sqrt(2) for 2, 3 */
  int diffusivity;                             /* 1 (PM_G2), the only one built */
} modsx_kaze_params;
typedef struct modsx_kaze_point {              /* a cv::KeyPoint of the detector's lists */
  float x, y, size, response;
  int octave, class_id;                        /* class_id: the level */
} modsx_kaze_point;
void modsx_default_kaze_params(modsx_kaze_params *p);
/* out: malloc'd (modsx_free) keypoints as the branch fills det_kp: x, y, response and s = size / 3.0 widened from the f32
 * cv::KeyPoint, a11 = cos(0.0), a12 = sin(0.0), a21 = -sin(0.0), a22 = cos(0.0), octave_number = octave, every other field 0.
 * Returns their number. */
int modsx_detect_kaze(modsx_ctx *ctx, const modsx_image *img, const modsx_kaze_params *par, modsx_keypoint **out);
/* The same for n_imgs images of any sizes with shared launches: out = the keypoints of image 0, then image 1, ...;
 * counts[i] = the number of image i.  Returns the total.  Each image's list equals what modsx_detect_kaze gives for it. */
int modsx_detect_kaze_batch(modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_kaze_params *par,
                            modsx_keypoint **out, int *counts);
/* host only: regions of KAZE keypoints as the branch leaves them -- type = MODSX_DET_KAZE, otherwise as modsx_surf_regions. */
int modsx_kaze_regions(const modsx_keypoint *kps, int n, int img_id, modsx_region *out);
/* host only: the level table for a rows x cols image.  levels [MODSX_KAZE_MAX_LEVELS][8] = (octave, sublevel, rows, cols,
 * sigma_size, derivative kernel size, derivative distance, FED steps); sigmas [.][2] = (esigma, etime); tau [.][MODSX_KAZE_MAX_TAU];
 * tiles [4] = (width, height of a stencil tile, positions of a scan tile, the largest derivative distance); *omax = the octaves that
 * survive the 80 x 40 rule.  Any output may be NULL.  Returns the number of levels, or MODSX_ERR_ARG as above. */
int modsx_kaze_geometry(int rows, int cols, const modsx_kaze_params *par, int *levels, float *sigmas, float *tau, int *tiles, int *omax);
/* Stage tap of one image.  kc [2] = (kcontrast, hmax); hist [kcontrast_nbins]; Lt, Lsmooth, Lflow, Ldet: the planes of every level,
 * one after the other in level order (Lflow of level 0 is zeros, Lsmooth of level 0 is Lt); then the lists: raw [cap][3] = (level,
 * row, col) with rawv [cap] the 3 x 3 maxima in scan order, aux after the same-level / lower-level pass, upper after the upper-level
 * pass, fin after refinement (the first cap records of each).  counts [4] = their lengths (call again with a larger cap when one
 * exceeds it).  Returns the number of levels. */
int modsx_debug_kaze(modsx_ctx *ctx, const modsx_image *img, const modsx_kaze_params *par, float *kc, long *hist, float *Lt, float *Lsmooth,
                     float *Lflow, float *Ldet, int *raw, float *rawv, modsx_kaze_point *aux, modsx_kaze_point *upper,
                     modsx_kaze_point *fin, int cap, int *counts);
/* The extrema scan, both filter passes and the refinement on caller-supplied Ldet planes (host memory, laid out as above for a rows
 * x cols image); lists and counts as modsx_debug_kaze.  Returns the number of levels. */
int modsx_debug_kaze_scan(modsx_ctx *ctx, int rows, int cols, const modsx_kaze_params *par, const float *ldet, int *raw, float *rawv,
                          modsx_kaze_point *aux, modsx_kaze_point *upper, modsx_kaze_point *fin, int cap, int *counts);
/* KAZE detector work of this context since modsx_create, cumulative (measurement hook): calls that launched, images, kernel
 * launches, diffusion steps launched, waits of the host for the device, raw maxima, survivors of the filter passes, keypoints,
 * microseconds the host spent in the filter passes and the refinement.  Fills out[0 .. min(n, 9) - 1], returns 9. */
int modsx_kaze_counters(modsx_ctx *ctx, long *out, int n);

/* ---- external affine adaptation: DetectAffineShape (synth-detection.cpp:922-1074) on a caller's regions ------------------
 * Baumberg iteration on the view image itself for a finished region list: what SynthDetectDescribeKeypoints runs
 * (imagerepresentation.cpp:1226-1236) in every detector branch that sets doExternalAffineAdaptation -- SURF with doBaumberg = 1
 * (imagerepresentation.cpp:1048), ORB, FAST, STAR, BRISK, KAZE, FOCI, SFOP, WAVE, WASH, TILDE-plugin.  The
 * library runs two of those detectors itself, SURF (modsx_detect_surf) and KAZE (modsx_detect_kaze: AKAZE's sources are in the
 * reference tree, only the OpenCV routines they call are not); the regions of the others come from the caller.  Per region, bit for bit:
 *   lx, ly    (float)det_kp.x, (float)det_kp.y on img (no pyramid, no pixelDistance)
 *   ratio     (float)(det_kp.s / (double)1.6f): the function's own constant, formed on the host in f64; no parameter replaces it
 *   border    interpolateCheckBorders(cols, rows, lx, ly, (float)a11 .. (float)a22, res, res) with res = (int)(2 * 5.0 * ratio)
 *             (truncated toward zero) and the region's OWN matrix: a region that fails is dropped without an iteration
 *   loop      from the identity (the input matrix takes part in the border test only), the AFF_BMBRG_SMM body of findAffineShape
 *             on the kernels of modsx_detect_affine_keypoints, one launch per call on the context's stream
 *   output    the converged regions in input order, det_kp.a11 .. a22 = the f32 shape widened to double, every other field as
 *             given; NaN, negative discriminant, anisotropy above 6 and the iteration limit drop the region.
 * The reference function ends without a return statement; these entries return the number of output regions.
 * Defaults (modsx_default_affshape_params): AffineShapeParams(), detectors/affinedetectors/affine.h:52-63 -- maxIterations 16
 * (:54), convergenceThreshold 0.05 (:56), smmWindowSize 19 (:58), affBmbrgMethod AFF_BMBRG_SMM (:61).
 * Refusals, MODSX_ERR_ARG with a message and before any launch: a null pointer or a negative count; smmWindowSize even or
 * outside 3..19; affBmbrgMethod other than 0 (AFF_BMBRG_HESSIAN needs cv::SVD and is built nowhere in this library); an image
 * below 4 x 4; a region whose x, y, s or matrix entries are not finite, or with |10 * ratio| >= 2^31 (the reference's conversion
 * to int is undefined there).  maxIterations has no upper limit: the kernels loop to it and keep no per-iteration storage.
 * Parameters and regions are checked first; then n == 0 or maxIterations <= 0 gives 0 regions (*out an empty array) without a
 * launch and without a look at the context or the image.  Pixels must be finite. */
typedef struct modsx_affshape_params {
  int maxIterations;            /* 16 */
  int smmWindowSize;            /* 19 */
  float convergenceThreshold;   /* 0.05 */
  int affBmbrgMethod;           /* 0 = AFF_BMBRG_SMM; 1 = AFF_BMBRG_HESSIAN is refused */
} modsx_affshape_params;
void modsx_default_affshape_params(modsx_affshape_params *p);
/* out: malloc'd (modsx_free).  Returns the number of regions. */
int modsx_detect_affine_shape(modsx_ctx *ctx, const modsx_image *img, const modsx_region *in, int n,
                              const modsx_affshape_params *par, modsx_region **out);
/* The same for n_imgs images in one launch: in = the counts[0] regions of image 0, then those of image 1, ...; out likewise with
 * out_counts[i] regions of image i.  Returns the total.  Each image's list equals what modsx_detect_affine_shape gives for it. */
int modsx_detect_affine_shape_batch(modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_region *in,
                                    const int *counts, const modsx_affshape_params *par, modsx_region **out, int *out_counts);
/* Test entry: the same job list and launch, reported per INPUT region -- border [.] = the up-front test, u [.][4] / ok / iters as
 * modsx_debug_baumberg reports them (the state and the loop counter when the loop was left; identity, ok = 0 and iters = -1 for
 * a border-refused region; identity, 0, 0 and no launch with maxIterations <= 0).  variant: -1 = what the entries above launch
 * (modsx_debug_baumberg_variant), 0..3 as modsx_debug_baumberg_geometry; geometry [4] = that of the launch over the regions
 * that passed the border test.  Returns the number of regions launched. */
int modsx_debug_affine_shape(modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_region *in, const int *counts,
                             const modsx_affshape_params *par, int variant, unsigned char *border, float *u, int *ok, int *iters,
                             int *geometry);
/* host only: ratio [n], res [n] (the truncated window argument) and border [n] (1 = refused) of every region on a cols x rows
 * image; any of the three may be NULL.  Returns n, or MODSX_ERR_ARG for a region or an image the entries above refuse. */
int modsx_affshape_jobs(const modsx_region *in, int n, int cols, int rows, float *ratio, int *res, unsigned char *border);
/* External adaptation work of this context since modsx_create, cumulative (measurement hook): calls, regions in, regions the
 * border test refused, regions launched, regions converged, launches.  Fills out[0 .. min(n, 6) - 1], returns 6. */
int modsx_affshape_counters(modsx_ctx *ctx, long *out, int n);

/* ---- CLAHE on the device: the drivers' doCLAHE step (engine_clahe.hip, kernels_clahe.hip) ---------------------------------
 * With `[Matching] doCLAHE` set every driver of the reference runs createCLAHE(), setClipLimit(4) and clahe->apply() on the
 * 8-bit gray image before it builds the ImageRepresentation (mods.cpp:139-189, mods_multi.cpp:162-178 for the query and every
 * partner, extract_features.cpp:92-103, export_descriptors.cpp:92-119).  These entries are that step on an uploaded image.
 * Contract: CLAHE_Impl::apply of OpenCV 2.4.9, modules/imgproc/src/clahe.cpp, restated here (no OpenCV is linked or needed; the
 * restatement is not pinned against an OpenCV build).  tx, ty = tiles_x, tiles_y; H = 256.
 *   source    the u8 value of a pixel is saturate_cast<uchar>(v) of the gray f32 value: round to nearest even, clamp to 0 .. 255,
 *             NaN -> 0.  A u8 upload is unchanged by it; a 3-channel upload has gone through (B + G + R) / 3.
 *   tiles     cols % tx == 0 && rows % ty == 0: tile = cols / tx x rows / ty on the image.  Otherwise the LUT source is the
 *             image padded with BORDER_REFLECT_101 by ty - rows % ty rows at the bottom and tx - cols % tx columns at the right
 *             (a divisible side is padded by a whole ty / tx), tile = padded size / grid.  No padded copy is made.
 *   scale     total = tileW * tileH; lutScale = (float)(H - 1) / total; clipLimit = clip_limit > 0 ?
 *             max((int)(clip_limit * total / H), 1) : 0 in f64 (a product of INT_MAX or more gives INT_MAX: nothing is clipped)
 *   per tile  hist[256] of the tile's ROI; with clipLimit > 0: clipped = sum max(hist[i] - clipLimit, 0), hist[i] =
 *             min(hist[i], clipLimit), batch = clipped / H, residual = clipped - batch * H, hist[i] += batch, hist[i]++ for
 *             i < residual; lut[i] = saturate_cast<uchar>((float)sum_i * lutScale) with the running int sum
 *   per pixel tyf = (float)y / tileH - 0.5f, ty1 = floor(tyf), ya = tyf - ty1, ty2 = ty1 + 1, then ty1 = max(ty1, 0), ty2 =
 *             min(ty2, ty - 1); the same in x; res = 0, res += lut[ty1, tx1][v] * ((1 - xa) * (1 - ya)), += lut[ty1, tx2][v] *
 *             (xa * (1 - ya)), += lut[ty2, tx1][v] * ((1 - xa) * ya), += lut[ty2, tx2][v] * (xa * ya) in f32 without contraction;
 *             dst = saturate_cast<uchar>(res), stored as f32: the integers 0 .. 255 that ImageRepresentation(img_clahe) holds.
 * variant 1 is the rule of OpenCV 3.x / 4.x (restated from memory of those sources): the residual is spread with a step
 * (step = max(H / residual, 1); for (i = 0; i < H && residual > 0; i += step, residual--) hist[i]++), txf = x * (1.0f / tileW)
 * - 0.5f (and in y), res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya with xa1 = 1.0f - xa.
 * Defaults (modsx_default_clahe_params): clip 4.0, 8 x 8 tiles, variant 0 -- what the drivers set (createCLAHE's own clip is 40).
 * Refusals, MODSX_ERR_ARG with a message and before any launch: a null pointer; tiles_x or tiles_y < 1; tiles_x * tiles_y above
 * MODSX_CLAHE_MAX_TILES (the LUT table of an image, tiles x 256 bytes, is staged in 64 KiB of LDS); clip_limit negative or not
 * finite; variant other than 0 / 1; an output of another size than its input; an image whose pixels are not memory of the
 * context's device; in a batch more than 65535 images, two outputs that share their pixels, an output that is another image's
 * input.  Images are one-channel by construction (modsx_image_wrap_device takes nothing else).  Not here: 16-bit input, colour
 * CLAHE; modsx_match_ladder / modsx_match_one_to_many do not equalise -- as in the reference the caller does it first. */
#define MODSX_CLAHE_MAX_TILES 256
typedef struct modsx_clahe_params {
  double clip_limit;            /* 4.0 */
  int tiles_x, tiles_y;         /* 8, 8 */
  int variant;                  /* 0 = OpenCV 2.4.9 (the reference's), 1 = OpenCV 3.x / 4.x */
} modsx_clahe_params;
void modsx_default_clahe_params(modsx_clahe_params *p);
/* out: an image of the same size; may be `in` itself (in place: the launches that read the image as LUT source are ordered
 * before the pixel pass).  Three launches on the context's stream; returns after they have finished. */
int modsx_image_clahe(modsx_ctx *ctx, const modsx_image *in, const modsx_clahe_params *par, modsx_image *out);
/* the same into a fresh handle (modsx_image_free); NULL on failure */
modsx_image *modsx_image_clahe_new(modsx_ctx *ctx, const modsx_image *in, const modsx_clahe_params *par);
/* n images of ANY sizes in one launch set: three launches for the whole batch, from a device table of per-image geometry
 * (mods_multi's loop over the partners).  out[i] may be in[i].  Every result equals that of a single call.  n == 0 is MODSX_OK. */
int modsx_image_clahe_batch(modsx_ctx *ctx, const modsx_image *const *in, modsx_image *const *out, int n, const modsx_clahe_params *par);
/* host only: what the launcher derives from the image size, from the function it calls itself.  out[0 .. 8] = tileW, tileH,
 * padded cols, padded rows, clipLimit, the bits of lutScale (f32), row strips per tile of the histogram launch, tile rows per
 * strip, workgroups of the pixel pass.  Strip rule: rows per strip = max(1, 4096 / tileW), raised so that a tile has at most
 * 256 strips and never above tileH; pixel pass: one workgroup per 4096 consecutive pixels.  Sizes 1 .. 16384 per side, at most 64 Mpx.  Returns 9. */
int modsx_clahe_geometry(int rows, int cols, const modsx_clahe_params *par, int *out);
/* Test entry: the first two launches on `in`; hist [tiles][256] = the counts of every tile BEFORE clipping, lut [tiles][256] =
 * the finished LUTs (either may be NULL), tiles in row-major order. */
int modsx_debug_clahe(modsx_ctx *ctx, const modsx_image *in, const modsx_clahe_params *par, int *hist, unsigned char *lut);
/* CLAHE work of this context since modsx_create, cumulative: calls (a batch is one), images, tiles, histogram strips, pixels,
 * launches.  Fills out[0 .. min(n, 6) - 1], returns 6. */
int modsx_clahe_counters(modsx_ctx *ctx, long *out, int n);

/* ---- the learned-descriptor front end: CAFFE patches and row norms (engine_caffe.hip, kernels_caffe.hip) -------------------
 * What the reference's "CAFFE" branch (imagerepresentation.cpp:1343-1534) does around its network: the input blob of the
 * regions of one image, and L2normalize / L1normalize / RootNormalize (:181-217) on the network's output rows.  The network
 * itself is the caller's (mods_amd/learned.py runs a torch module between the two on the same device).  Unlike
 * DescribeRegions<> the branch samples the ORIGINAL image at the REPROJECTED frame, blurs nothing, normalises nothing
 * photometrically, keeps colour, takes any odd patch size, rounds to bytes and subtracts a per-channel mean.
 *   input     planes[c]: 1 or 3 modsx_image handles of equal size on the context's device.  Three are the B, G, R planes of
 *             cv::split(OriginalImg) after convertTo(CV_32FC3), each uploaded with modsx_image_upload(.., channels = 1, ..);
 *             one is a gray OriginalImg.  regs[n]: only reproj_kp is read (regions after modsx_reproject_regions).
 *   frame     patchImageSize = 2 * (int)mrSize + 1; imageToPatchScale = (double)patchImageSize / (double)patchSize;
 *             curr_sc = (float)(imageToPatchScale * reproj_kp.s), an f64 product rounded once; the arguments of interpolate are
 *             (float)x, (float)y, (float)a11 * curr_sc, (float)a12 * curr_sc, (float)a21 * curr_sc, (float)a22 * curr_sc (f32
 *             products) and a P x P result, P = patchSize.
 *   samples   interpolate, detectors/helpers.cpp:551-626, on every plane: interpolateCheckBorders false -> the (int)
 *             truncation branch, true -> floor + bounds test with 0 outside; the serial f32 running sums of the row starts
 *             (rx += a12, ry += a22) and along a row (WX += a11, WY += a21), no multiplication by the index, no contraction.
 *             The coordinates are the same for the three planes.
 *   bytes     saturate_cast<uchar>(float): round to nearest, ties to even, clamp to 0 .. 255 (convertTo(CV_8UC3) / CV_8U).  A
 *             gray input puts its one byte into all three channels (GRAY2BGR).
 *   blob      out[i][c][h][w] = (float)byte - (float)(int)mean[c]: mean_px is a std::vector<int> assigned from doubles, so the
 *             mean is truncated toward zero; the layout is CVMatToDatum's, channel-major f32 [n][3][P][P].
 *   flags     optional, [n] u8 on the host: bit 0 = interpolateCheckBorders was true (the border branch ran); bit 1 = at least
 *             one sample fell outside -- what interpolate returns and the branch ignores.
 * Where the reference is broken: (1) the branch is #ifdef WITH_CAFFE and names CaffeDescParam.patchSize / .mrSize, which
 * GetCaffePars writes but the struct holds in PEParam -- the contract is the text of the branch; (2) with an even patchSize
 * interpolate writes (2 (P >> 1) + 1)^2 floats into a P x P Mat and overruns it -- refused; (3) blob_proto is never cleared
 * between batches (:1475), so from its second batch on the reference feeds sums of patches -- not reproduced, every region
 * gets what the reference gives a region of its FIRST batch; (4) neither OpenCV nor Caffe is linked: the rounding rule and the
 * CHW layout are restated, not pinned, as CLAHE's.
 * Defaults (modsx_default_caffe_params): mrSize 3 sqrt(3) and patchSize 41 (PatchExtractionParams), mean {104, 117, 123} in
 * B, G, R order.  n is the caller's batch (the reference uses 256).  Both forms return after the work has finished.
 * Refusals, MODSX_ERR_ARG with a message and before any launch: n < 0 or a null pointer; patchSize even or outside 1 ..
 * MODSX_CAFFE_MAX_PATCH; mrSize not finite, negative or above 1e6; a mean that is not finite or outside +-2^30; a plane count
 * other than 1 or 3; planes of different sizes or of another device; a device blob that is not 4-byte aligned.  n == 0
 * succeeds and writes nothing.  Non-finite pixels and non-finite reproj_kp fields are outside the contract (every load stays
 * inside the planes; a pixel whose rounded value leaves the int range clamps like any other).
 * Not here: network inference; CAFFE in modsx_rep_describe_append, the ladder, modsx_rep_add_views or the sharded path; a
 * 1-channel blob; even patch sizes; DoSIFTLikeOrientation at a patch size other than 41 (run modsx_detect_orientation and
 * modsx_reproject_regions first); `Pooling`, which GetCaffePars reads and nothing uses. */
#define MODSX_CAFFE_MAX_PATCH 255
#define MODSX_CAFFE_MAX_DIM 4096
enum { MODSX_CAFFE_NORM_L2 = 0, MODSX_CAFFE_NORM_L1 = 1, MODSX_CAFFE_NORM_ROOTL2 = 2, MODSX_CAFFE_NORM_NONE = 3 };
typedef struct modsx_caffe_params {
  double mrSize;                /* 3 sqrt(3) */
  int patchSize;                /* 41 */
  double mean[3];               /* 104, 117, 123: B, G, R */
} modsx_caffe_params;
void modsx_default_caffe_params(modsx_caffe_params *p);
/* blob: [n][3][P][P] f32 on the host; flags: [n] u8 on the host or NULL.  Returns n. */
int modsx_caffe_patches(modsx_ctx *ctx, const modsx_image *const *planes, int n_planes, const modsx_region *regs, int n,
                        const modsx_caffe_params *par, float *blob, unsigned char *flags);
/* the same with the blob in HBM: dev_blob is a dense [n][3][P][P] f32 device pointer, 4-byte aligned */
int modsx_caffe_patches_device(modsx_ctx *ctx, const modsx_image *const *planes, int n_planes, const modsx_region *regs, int n,
                               const modsx_caffe_params *par, void *dev_blob, unsigned char *flags);
/* host only: what the launcher's job table holds for planes of rows x cols, from the function that fills it.  out [n][8] f32 =
 * curr_sc, the six arguments of interpolate (x, y, a11, a12, a21, a22) and interpolateCheckBorders (0 or 1).  Returns n. */
int modsx_caffe_jobs(const modsx_region *regs, int n, const modsx_caffe_params *par, int rows, int cols, float *out);
/* host only: the work split of a launch over n regions at patchSize: out[0 .. 6] = workgroups, wavefronts per workgroup (one
 * lane per patch row), column chunks per patch, columns per chunk (at most 64), LDS byte stride of a tile row, LDS bytes of a
 * workgroup with one plane, the same with three.  Returns 7. */
int modsx_debug_caffe_geometry(int n, int patchSize, int *out);
/* The norms on [n][dim] f32 rows, 1 <= dim <= MODSX_CAFFE_MAX_DIM, exactly imagerepresentation.cpp:181-217.
 *   L2      norm (f64) += (double)(x[i] * x[i]) with the product rounded to f32 first, i = 0 .. dim - 1 in that order; coef =
 *           1.0 / sqrt(norm); out[i] = (float)floor(512.0 * coef * (double)x[i]), evaluated left to right
 *   L1      norm += (double)x[i] -- the signed sum, the reference takes no absolute value; coef = 1.0 / norm; the same floor
 *   ROOTL2  the L1 sum, out[i] = (float)sqrt(512.0 * coef * (double)x[i]) (the L2 pass RootNormalize runs first is overwritten)
 *   NONE    a copy
 * f64 division and square root are the IEEE ones.  A zero norm gives NaN / +-inf rows and a negative product NaN, as in the
 * reference: they are returned as such and are outside the matcher's contract.  The device form takes 4-byte aligned dense rows;
 * dev_out may be dev_rows.  MODSX_ERR_ARG before any launch: n < 0, a null pointer, dim or norm out of range, a misaligned
 * device pointer; n == 0 succeeds and writes nothing.  Returns n. */
int modsx_caffe_norm_rows(modsx_ctx *ctx, const float *rows, int n, int dim, int norm, float *out);
int modsx_caffe_norm_rows_device(modsx_ctx *ctx, const void *dev_rows, int n, int dim, int norm, void *dev_out);
/* Front-end work of this context since modsx_create, cumulative: patch calls, regions, regions on the border branch, launches
 * (norm launches included).  Fills out[0 .. min(n, 4) - 1], returns 4. */
int modsx_caffe_counters(modsx_ctx *ctx, long *out, int n);

/* ---- float descriptor classes of a stored representation (engine_reps_f32.hip) -------------------------------------------
 * A modsx_rep also holds one class per (detector in {MODSX_DET_HESSIAN, MODSX_DET_MSER, MODSX_DET_SURF}) x (float descriptor
 * type MODSX_DESC_CAFFE .. MODSX_DESC_SURF), as RegionVectorMap[det][desc] does for any descriptor name.  Widths: CAFFE any
 * dim % 4 == 0 in [4, MODSX_FGINN32_MAX_DIM] (learned vectors), DAISY a width modsx_daisy_dim can return, LIOP 144, MROGH 192,
 * SURF 64; MROGH rows come from the caller only, CAFFE rows from the caller's network (modsx_caffe_patches in front of it,
 * modsx_caffe_norm_rows and modsx_rep_append_f32_device behind it).  A class fixes its width at its first append; a later append of
 * another width is MODSX_ERR_ARG.
 *   Stored form.  A class keeps its rows in the row form of the f32 matcher (the kernel width DK floats per row, zero behind
 * dim, 16-byte aligned) padded with zero rows to a multiple of 256 rows, and the positions reproj_kp.x, y of its regions as
 * [n][2] f64 in HBM: the form both the query side and the train side of a match read, so no stored match packs anything.  An
 * append writes its rows behind the old ones; the buffer starts at MODSX_REP_F32_FIRST_ROWS rows and grows x4, copying the
 * old rows once.  Values must be finite with |x| <= 1e17 (the matcher's contract): host rows are checked on the host, rows of
 * a device extractor through the flag word of the kernel that stores them.  An append that fails leaves the class as it was.
 * A class holds at most 2 000 000 regions.  The u8 classes and every entry that takes them are unchanged. */
#define MODSX_REP_F32_FIRST_ROWS 4096
/* LoadRegions for a float class: n regions and their dense [n][dim] f32 rows, ids as given.  Returns n.  MODSX_ERR_ARG: a
 * detector or type that names no float class, a width the type does not have or the class does not hold, an invalid value,
 * more than 2 000 000 regions in the class. */
int modsx_rep_append_f32(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs, const float *rows,
                         int dim, int n);
/* The same with the rows in HBM: dev_rows is a dense [n][dim] f32 device pointer, 4-byte aligned (rows a network or
 * modsx_caffe_norm_rows_device left there).  The same checks, the same stored form and the same results as the host entry on
 * the same values; the validity of the values is checked by the kernel that stores them. */
int modsx_rep_append_f32_device(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs,
                                const void *dev_rows, int dim, int n);
/* Describes the caller's (oriented) regions of one view image with the class's extractor -- MODSX_DESC_SURF, MODSX_DESC_LIOP
 * or MODSX_DESC_DAISY (CAFFE and MROGH are refused) -- and appends regions and rows; the rows stay on the device from the
 * extractor's kernel to the class.  They are bit for bit what modsx_describe_regions_surf / _liop / _daisy return for the same
 * arguments.  daisy_par = {rad, radq, thq, histq, nrm_type} for DAISY, NULL otherwise.  A region list that gives an invalid
 * row (SURF's NaN rows) is MODSX_ERR_ARG and leaves the class unchanged.  Returns n. */
int modsx_rep_describe_append(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_image *img,
                              const modsx_region *regs, int n, double mrSize, int patchSize, int fast_extraction, int photoNorm,
                              const int *daisy_par);
/* The regions and dense [n][dim] f32 rows of one float class as malloc'd copies (modsx_free), and its width (0 while the class
 * is empty); any pointer may be NULL.  Returns n. */
int modsx_rep_class_f32(modsx_ctx *ctx, const modsx_rep *rep, int detector, int desc_type, modsx_region **regs, float **rows, int *dim);
/* Stage tap: the MatchFlannFGINN records of one float class, rep1 the queries, rep2 the trains -- what modsx_match_fginn_f32
 * returns for the same rows and the positions reproj_kp.x, y of rep2's regions. */
int modsx_rep_match_fginn_f32(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *rep2, int detector, int desc_type, double ratio,
                              double contradDist, int nn, modsx_tentative **out);
/* Stage tap of the grouped launch set: the class of rep1 against that class of 1 <= G <= 4 partners in ONE launch set (one
 * search launch and one merge launch for all partners, one copy of every partner's four nearest keys, the host's walk, ONE
 * resolve launch for the walks of all partners that are still open, one copy back).  outs[g] (modsx_free) / counts[g]: partner
 * g's records, those of modsx_rep_match_fginn_f32(rep1, reps2[g]).  Partners with an empty class are left out of the launches.
 * Returns G. */
int modsx_rep_match_group_f32(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, int detector, int desc_type,
                              double ratio, double contradDist, int nn, modsx_tentative **outs, int *counts);
/* modsx_match_reps also takes float classes in classes[]; with n_classes == 0 it includes every float class that is non-empty
 * in rep1, with par->match_ratio.  A float class costs one grouped launch set per group of partners.  The database
 * attachment applies to RootSIFT only.  Classes are concatenated in std::map order of the reference's names -- descriptor
 * CAFFE, DAISY, HalfRootSIFT, HalfSIFT, LIOP, MROGH, RootSIFT, SIFT, SURF, then detector HessianAffine, MSER, SURF -- and the
 * region indices of a result refer to that concatenation.
 * host only: the position of a class in that order, -1 when there is no such descriptor type or detector. */
int modsx_rep_class_rank(int detector, int desc_type);
/* host only, no context: the train axis of the grouped launch set for n1 queries against G <= 4 partners of n2[g] rows.
 * geometry[4] = {tile length, kernel width DK, query blocks gx, splits in all}; per_problem [G][3] = {tiles, splits, tiles per
 * split} (zeros for an empty partner); splits [cap][3] = {partner, first tile, end tile} of the first min(cap, splits) splits
 * in launch order (may be NULL with cap 0).  Returns the number of splits.  Every partner with n2 >= 1 has the S and tiles per
 * split modsx_debug_fginn32_geometry(n1, n2[g], dim, 0) gives it alone, whatever shares the launch. */
int modsx_debug_fginn32_group_geometry(int n1, const int *n2, int G, int dim, int *geometry, int *per_problem, int *splits, int cap);
/* cumulative on this context: grouped launch sets, problems in them, queries sent to resolve, resolve launches.  Fills
 * out[0 .. min(n, 4) - 1], returns 4. */
int modsx_fginn32_group_counters(modsx_ctx *ctx, long *out, int n);

/* ---- binary descriptor classes of a stored representation (engine_reps_bin.hip) ------------------------------------------
 * A modsx_rep also holds one class per (detector in {MODSX_DET_HESSIAN, MODSX_DET_MSER, MODSX_DET_ORB, MODSX_DET_SURF}) x
 * (binary descriptor type MODSX_DESC_BRISK, MODSX_DESC_FREAK, MODSX_DESC_ORB): the classes MatchImgReps matches with
 * MatchFLANNDistance (see modsx_match_hamming for the search and the record rule).  A class takes any width
 * 1 <= nbytes <= MODSX_HAMMING_MAX_BYTES and fixes it at its first append; a later append of another width is MODSX_ERR_ARG.
 * The library does not extract such descriptors: the rows come from the caller, e.g. from modsx_load_regions.
 *   Stored form.  A class keeps its rows exactly as the pack kernel of the Hamming search writes them: WK dwords per row (WK =
 * the kernel width, ceil(nbytes / 4) rounded up to 1, 2, 4, 8 or 16), zero behind nbytes, the array 16-byte aligned, zero rows
 * up to the capacity.  The capacity is a multiple of 1024 rows -- whole 256-query workgroups and whole train tiles at every WK --
 * so the same buffer is the query side and the train side of any match and nothing is packed at match time.  An append packs
 * its rows behind the old ones; the buffer starts at MODSX_REP_BIN_FIRST_ROWS rows and grows x4, copying the old rows once.
 * The search never visits a row at or behind the class's count, so a zero padding row is never a neighbour.  An append that
 * fails leaves the class as it was; a class that is still empty afterwards keeps no buffer.  A class holds at most 2 000 000
 * regions.  The u8 and float classes and every entry that takes them are unchanged. */
#define MODSX_REP_BIN_FIRST_ROWS 4096
/* LoadRegions for a binary class: n regions and their dense [n][nbytes] rows, ids as given.  dtype 0 = u8, 1 = f32 holding the
 * integers 0..255; anything else is MODSX_ERR_ARG (the rule of modsx_match_hamming).  Returns n; n == 0 is a no-op that returns
 * 0.  MODSX_ERR_ARG: a detector or type that names no binary class, nbytes outside 1..64 or another width than the class holds,
 * an invalid value, more than 2 000 000 regions in the class, a representation on another device. */
int modsx_rep_append_bin(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs, const void *desc,
                         int nbytes, int dtype, int n);
/* The same from dense [n][nbytes] u8 rows that already live in HBM (any alignment); the regions come from the host. */
int modsx_rep_append_bin_device(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs,
                                const void *dev_desc_u8, int nbytes, int n);
/* The regions and dense [n][nbytes] u8 rows of one binary class as malloc'd copies (modsx_free), and its width (0 while the
 * class is empty); any pointer may be NULL.  Returns n. */
int modsx_rep_class_bin(modsx_ctx *ctx, const modsx_rep *rep, int detector, int desc_type, modsx_region **regs, unsigned char **desc_u8,
                        int *nbytes);
/* Stage tap: the MatchFLANNDistance records of one binary class, rep1 the queries, rep2 the trains -- what
 * modsx_match_hamming_device returns for the same rows. */
int modsx_rep_match_hamming(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *rep2, int detector, int desc_type,
                            double distanceThreshold, modsx_tentative **out);
/* Stage tap of the grouped launch set: the class of rep1 against that class of 1 <= G <= 4 partners in ONE launch set (one
 * search launch and one merge launch for all partners, one copy of G x n1 x 16 bytes back; the Hamming search has no walk and no
 * resolve pass).  outs[g] (modsx_free) / counts[g]: partner g's records, those of modsx_rep_match_hamming(rep1, reps2[g]).
 * Partners with an empty class give 0 records and are left out of the launches.  Returns G.
 *   Refusals of both taps and of modsx_match_reps for a binary class, all MODSX_ERR_ARG before any launch: a train class of
 * exactly one region in ANY partner (the reference reads a second neighbour that was never written), distanceThreshold <= 0 or
 * not finite, widths that differ between the two representations, a (detector, type) pair that names no binary class, a
 * representation on another device, G outside 1..4. */
int modsx_rep_match_group_hamming(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, int detector,
                                  int desc_type, double distanceThreshold, modsx_tentative **outs, int *counts);
/* modsx_match_reps takes binary classes in classes[], with the class's DistanceThreshold in the `ratio` field.  With
 * n_classes == 0 binary classes are NOT included: modsx_pair_params has no distance threshold, and the reference matches a class
 * only if its section gives one.  A binary class costs one grouped launch set per group of partners; the pair tail is that of
 * modsx_match_regions_hamming (DuplicateFiltering with key = ratio, NaN from 0 / 0 as it is there, then LORANSACFiltering).
 * Classes are concatenated in the order of modsx_rep_class_order.
 * host only: the position of a class in the std::map order of the reference's names over every (descriptor, detector) name pair
 * -- descriptor BRISK, CAFFE, DAISY, FREAK, HalfRootSIFT, HalfSIFT, LIOP, MROGH, ORB, RootSIFT, SIFT, SURF, then detector
 * HessianAffine, MSER, ORB, SURF: 4 x the descriptor's place + the detector's -- or -1 for a pair that names no class of a
 * representation.  modsx_rep_class_rank is unchanged and does not know the binary classes; on the 27 classes it knows, the two
 * functions agree in relative order. */
int modsx_rep_class_order(int detector, int desc_type);
/* host only, no context: the table the grouped launch set would use for n1 queries against G <= 4 partners of n2[g] rows of
 * nbytes bytes.  geometry[4] = {tile length in trains, kernel width WK, query blocks, splits in all}; per_problem [G][3] =
 * {tiles, splits, tiles per split} (zeros for an empty partner); splits [cap][3] = {partner, first tile, end tile} of the first
 * min(cap, splits) splits in launch order (may be NULL with cap 0).  Returns the number of splits.  Every partner with rows has
 * the S and tiles per split modsx_debug_hamming_geometry(n1, n2[g], nbytes, 0) gives it alone, whatever shares the launch. */
int modsx_debug_hamming_group_geometry(int n1, const int *n2, int G, int nbytes, int *geometry, int *per_problem, int *splits, int cap);
/* cumulative on this context: grouped launch sets, problems in them, rows packed by appends, pack launches issued at match time
 * (0 for stored matches).  Fills out[0 .. min(n, 4) - 1], returns 4. */
int modsx_hamming_group_counters(modsx_ctx *ctx, long *out, int n);

/* Measurement hooks (no reference counterpart; the reference only keeps wall-clock TimeLog, structures.hpp:51-74).
 * modsx_profile(ctx, 1) brackets every kernel launch with HIP events on the ctx stream and accumulates, per kernel
 * class, GPU milliseconds, launch count and algorithmic work (bytes; flops for the matcher).  Classes in order:
 * blur_hess, hessian, resize, nms_localize (scan + refine), baumberg, orientation, patch_sample, blur_rows, describe,
 * match_fginn, gray, warp_affine, view_blur, blur_cols, match_sweep1 (the one k_match launch that carries the 2 N M 128
 * contraction; also part of match_fginn), match_db (k_dbnn_min, the database pass of the _db matchers: 2 x selected queries x
 * database rows x 128; not part of match_fginn).  modsx_kernel_stats returns the number of classes.
 * Cost: with ROCm 7 a stream that has recorded timing events keeps per-dispatch completion signals on its queue -- every later
 * launch of that context costs its host thread more CPU (measured: 8.5 -> 29 ms per 1920x1080 pair of ~220 launches), also after
 * modsx_profile(ctx, 0).  Profile on contexts made for it, or after the throughput measurement (bench.py orders its legs so). */
int modsx_profile(modsx_ctx *ctx, int enable);
int modsx_kernel_stats(modsx_ctx *ctx, double *ms, double *work, long *launches, int n);

#ifdef __cplusplus
}
#endif
#endif
