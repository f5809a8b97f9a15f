// engine_api.hpp -- functions shared between engine.hip, engine_detect.hip, engine_views.hip, engine_shard.hip, describe_plan.cpp,
// ransac.cpp, filters.cpp and capi.hip.  Of the stored representations it holds the slot structures, the class identity
// (RepClassId; the table behind it is engine_reps.hip), to_malloc and the group-geometry report; the host's FGINN walk on f32 keys
// comes in through engine.hpp from fginn_walk.hpp.
#pragma once
#include <stdio.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>
#include "engine.hpp"

struct modsx_comm;

namespace mx {
const char *last_error();
void prof_collect(modsx_ctx *c);
void prof_reset(modsx_ctx *c, bool enable);
modsx_ctx *ctx_create(int device_id);
void ctx_destroy(modsx_ctx *c);
int build_pyramids(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_hessaff_params &p,
                   bool singleOctaveFromFirstLevel);
int detect_scalespace_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_hessaff_params &p,
                            std::vector<modsx_sskp> *out);
int detect_keypoints_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_hessaff_params &par,
                           const double *tilts, const double *zooms, std::vector<modsx_keypoint> *out);
int debug_pyramids(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_hessaff_params &p, int *geo, float *planes,
                   unsigned long long capFloats, unsigned long long *needFloats);
int debug_scan_levels(modsx_ctx *c, const float *resps, const float *blurs, int L, int rows, int cols, const modsx_hessaff_params &p,
                      std::vector<Candidate> &cands, std::vector<modsx_sskp> &out);
int debug_baumberg_geometry(modsx_ctx *c, int n, int W, int variant, int chunk, int *geo);
int debug_baumberg(modsx_ctx *c, const modsx_image *const *planes, int nplanes, const int *planeOf, const float *xyspd, int n,
                   const modsx_hessaff_params &p, int variant, int chunk, float *u, int *ok, int *iters, int *geo, int *handedOut);
// DetectAffineShape (synth-detection.cpp:922-1074) on a caller's regions (engine_detect.hip).  affshape_check / affshape_jobs: the
// refusals and the per-region host work that need no device (ratio, truncated window argument, up-front border test; each output
// optional); fn names the entry in the error text.  affine_shape_batch: in = the regions of image 0, then image 1, ... (counts per
// image); variant -1 = the production rule; out (optional) [nImgs]: the converged regions of every image; rep (optional): the
// per-INPUT-region report of modsx_debug_affine_shape.  Returns the number of regions launched or a negative status.
struct AffShapeReport { unsigned char *border; float *u; int *ok; int *iters; int *geo; };
int affshape_check(const char *fn, const modsx_affshape_params &p);
int affshape_jobs(const char *fn, const modsx_region *in, int n, int cols, int rows, float *ratio, int *res, unsigned char *border);
int affine_shape_batch(modsx_ctx *c, const char *fn, const modsx_image *const *imgs, int nImgs, const modsx_region *in, const int *counts,
                       const modsx_affshape_params &p, int variant, std::vector<modsx_region> *out, const AffShapeReport *rep);
// CLAHE (engine_clahe.hip).  clahe_check: the parameter refusals; clahe_geometry: tile and padded size, clipLimit, lutScale and the
// work split of one image -- the function the launcher itself sizes its table and grids with (both need no device; fn names the
// entry in the error text).  clahe_batch: n images of any sizes in one launch set on c->stream, out[i] may be in[i]; with out ==
// nullptr the pixel pass is left out (modsx_debug_clahe) and dbgHist [tiles][256] / dbgLut [tiles][256] (host, n == 1) are filled.
struct ClaheGeo { int tileW, tileH, padW, padH, clipLimit; float lutScale; int strips, stripRows, applyBlocks; };
int clahe_check(const char *fn, const modsx_clahe_params &p);
int clahe_geometry(const char *fn, int rows, int cols, const modsx_clahe_params &p, ClaheGeo &g);
int clahe_batch(modsx_ctx *c, const char *fn, const modsx_image *const *in, modsx_image *const *out, int n, const modsx_clahe_params &p,
                int *dbgHist, unsigned char *dbgLut);
// The learned-descriptor front end (engine_caffe.hip).  caffe_check / caffe_norm_check: the refusals that need no device (fn names
// the entry in the error text); caffe_jobs: the per-region host work -- the function that fills the launcher's job table.
// caffe_patches: blob [n][3][P][P] f32 on the host, or a device pointer (4-byte aligned) when onDevice; flags [n] u8 on the host or
// null.  caffe_norm_rows: rows / out on the host, or device pointers when onDevice (out may be rows).  Both return after the work.
int caffe_check(const char *fn, const modsx_caffe_params &p);
int caffe_norm_check(const char *fn, int n, int dim, int norm);
void caffe_jobs(const modsx_region *regs, int n, const modsx_caffe_params &p, int rows, int cols, CaffeJob *jobs);
int caffe_patches(modsx_ctx *c, const char *fn, const modsx_image *const *planes, int nplanes, const modsx_region *regs, int n,
                  const modsx_caffe_params &p, float *blob, bool onDevice, unsigned char *flags);
int caffe_norm_rows(modsx_ctx *c, const char *fn, const float *rows, int n, int dim, int norm, float *out, bool onDevice);
void detect_affine_regions(const modsx_keypoint *kps, int n, int img_id, int det_type, modsx_region *out);
// reproj (optional, one entry per image): what the caller's reproject_regions will be called with.  A region that
// reproject_certain_drop flags for it is treated like one at the view's border: no orientation job and no output entry,
// also under addUpRight (MODSX_ORI_PREFILTER=0 switches this off)
struct OriReproj { const double *H; int orig_w, orig_h; };
int detect_orientation_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const std::vector<modsx_region> *in,
                             double mrSize, int patchSize, int doHalfSIFT, int maxAngNum, double th, int addUpRight,
                             std::vector<modsx_region> *out, const OriReproj *reproj = nullptr);
int reproject_regions(modsx_region *regs, int n, const double *H, int orig_w, int orig_h);
int reproject_regions_box(modsx_region *regs, int n, const double *H, int orig_w, int orig_h, double boxk);
// drop[i] = 1: reproject_regions_box removes region i whatever rotation is applied to its shape first (engine.hip)
void reproject_certain_drop(const modsx_region *regs, int n, const double *H, int orig_w, int orig_h, double boxk, unsigned char *drop);
void orientation_counts(unsigned long long *launched, unsigned long long *skipped, bool reset);
void orientation_launches(unsigned long long *ldsTable, unsigned long long *globalTable, bool reset);
// The descriptor classes one step carries (modsx_pair_params / modsx_ladder_step n_desc, desc_types, desc_ratios resolved):
// `Descriptors=` and `FGINNThreshold=` of a [DetectorN] section.  half(): the step orients with doHalfSIFT = true
// (imagerepresentation.cpp:693-706, 1259-1264).
struct DescSet {
  int n = 1;
  int type[MODSX_MAX_DESC] = {MODSX_DESC_ROOT_SIFT, 0, 0, 0};
  double ratio[MODSX_MAX_DESC] = {0, 0, 0, 0};
  bool forceHalf = false;   // a caller that takes only the first class of a longer list keeps the list's orientation mode
  bool half() const { for (int i = 0; i < n; i++) if (type[i] >= 2) return true; return forceHalf; }
  int packed() const { int p = 0; for (int i = 0; i < n; i++) p |= (type[i] & 15) << (4 * i); return p; }
};
// rc = MODSX_ERR_ARG for a type outside 0..3, a type listed twice or n_desc outside 0..4
int resolve_descs(const modsx_pair_params &pp, const modsx_ladder_step *st, DescSet &ds);
void desc_class_order(const DescSet &ds, int *ord);   // the classes in descriptor-name order (GetCorresponcesVector)
// devU8x (optional): devU8x[k][i] receives the u8 descriptors of class k + 1 of image i (default: c->descU8x[k][i])
int describe_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const std::vector<modsx_region> *regs,
                   double mrSize, int patchSize, int fast, int photoNorm, int descType, double maxBin,
                   float *const *descHost, float *const *devF, uint8_t *const *devU8, const DescSet *ds = nullptr,
                   uint8_t *const *const *devU8x = nullptr);
// What follows a chunk's sampling and blur launches in place of k_describe (engine_liop.hip): run() gets the chunk's jobs and
// tables on the device and launches on c->stream.  describe_batch_tail is describe_batch for one image's regions with such a
// tail: the same windows, the same chunk planner, the same launch sets in front of it.
struct DescTail {
  int (*run)(modsx_ctx *c, void *self, const DescJob *jobs, int n, const float *grid, const int *needTab, const float *coordTab,
             int photoNorm);
  void *self;
};
int describe_batch_tail(modsx_ctx *c, const modsx_image *img, const std::vector<modsx_region> &regs, double mrSize, int patchSize,
                        int fast, int photoNorm, const DescTail &tail);
// The descriptors that are one kernel per normalised 41 x 41 patch (engine_patchdesc.hip).  launch() runs the kernel on s over nb
// patch rows: `first` is the index of the first of them within the call, out the output base (the rows' own when jobs is null,
// the call's when the jobs carry their output rows).  batchEnv names the variable that sets the patches per sub-batch.
struct PatchDesc {
  int dim;                  // descriptor width in floats
  const char *batchEnv;
  void (*launch)(void *self, hipStream_t s, const float *patches, int nb, int first, float *out, const DescJob *jobs);
  void *self;
};
// Both enqueue on c->stream and add their sub-batches to *subBatches; inside CtxBusy, n > 0.  The caller then runs patch_sync (the
// call's one wait and error check), books its counters, and patch_fetch copies the staged rows to a host caller
int patchdesc_patches(modsx_ctx *c, const PatchDesc &d, const float *patches, int n, float *desc, bool onDevice, long *subBatches);
int patchdesc_regions(modsx_ctx *c, const PatchDesc &d, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                      int patchSize, int fast, int photoNorm, float *desc, bool onDevice, long *subBatches);
int patch_sync(modsx_ctx *c);
int patch_fetch(modsx_ctx *c, float *rows, size_t floats, bool onDevice);
// LIOP and the normalised patches (engine_liop.hip).  out / patches: host pointers, or device pointers (4-byte aligned) when
// onDevice; dbgPath [n] / dbgPerm [n][673] (host, optional): modsx_debug_liop
int liop_tables(int patchSize, int *pixels, double *sx, double *sy, int cap);
int extract_patches(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                    int photoNorm, float *patches, bool onDevice);
int liop_patches(modsx_ctx *c, const float *patches, int n, int patchSize, float *desc, bool onDevice, int *dbgPath, int *dbgPerm);
int describe_regions_liop(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                          int photoNorm, float *desc, bool onDevice);
// Raw SIFT histograms, the f32 SIFT norm and DSP-SIFT (engine_dsp.hip).  hist / rows / out / desc: [n][128] f32, host pointers, or
// device pointers (4-byte aligned) when onDevice
int describe_regions_raw(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                         int photoNorm, float *hist, bool onDevice);
int sift_norm_rows(modsx_ctx *c, const float *rows, int n, double maxBinValue, float *out, bool onDevice);
int describe_regions_dspsift(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize,
                             int fast, int photoNorm, int numScales, double startCoef, double endCoef, double maxBinValue, float *desc,
                             bool onDevice);
// SURF (engine_surf.hip).  patches [n][41][41] f32 / desc [n][64] f32: host pointers, or device pointers (4-byte aligned) when
// onDevice.  surf_check_args: the refusals that need no device (patchSize, mrSize), made by the entries of capi.hip before they
// call in here; fn names the entry in the error text
int surf_tables(int patchSize, double mrSize, int *sample_x24, int *sample_y24, float *w1, float *w2, int *haar_size);
int surf_check_args(const char *fn, int patchSize, double mrSize);
int surf_patches(modsx_ctx *c, const float *patches, int n, double mrSize, float *desc, bool onDevice);
int describe_regions_surf(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                          int photoNorm, float *desc, bool onDevice);
// The SURF detector (engine_surfdet.hip).  surfdet_normalise: saveParameters; surfdet_geometry: layers [12][4] (may be null) = (width,
// height, step, filter), returns their number or MODSX_ERR_ARG for a layer of width or height 0; surfdet_check: the refusals of the
// entries that need no device; fn names the entry in the error text.  out [n]: the keypoints of every image in push order
modsx_surfdet_params surfdet_normalise(const modsx_surfdet_params &p);
int surfdet_geometry(const char *fn, int rows, int cols, const modsx_surfdet_params &par, int *layers);
int surfdet_check(const char *fn, const modsx_image *const *imgs, int n, const modsx_surfdet_params &par);
void surf_regions(const modsx_keypoint *kps, int n, int img_id, modsx_region *out);
int detect_surf_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_surfdet_params &par, std::vector<modsx_keypoint> *out);
int debug_surfdet(modsx_ctx *c, const modsx_image *img, const modsx_surfdet_params &par, float *integral, int *layers, float *resp,
                  unsigned char *lap, int *ext, double *dD, double *H, double *x, int *accepted, int *laplacian, int capExt, int *nExt);
// The KAZE detector (engine_kaze.hip).  kaze_geometry: the level table of Allocate_Memory_Evolution with every tau list, and the
// refusals that need no device (fn names the entry in the error text); returns the number of levels.  KazeTap: what modsx_debug_kaze
// reads of one image; KazeLists: the lists of Find_Scale_Space_Extrema and Do_Subpixel_Refinement, records as modsx.h lays them out
struct KazeLevel { int octave, sublevel, rows, cols, sigma_size, dsize, ksize, nsteps; float esigma, etime; std::vector<float> tau; };
int kaze_geometry(const char *fn, int rows, int cols, const modsx_kaze_params &par, std::vector<KazeLevel> &lv, int *omax);
void kaze_regions(const modsx_keypoint *kps, int n, int img_id, modsx_region *out);
struct KazeLists { std::vector<int> raw; std::vector<float> rawv; std::vector<modsx_kaze_point> aux, upper, final; };
struct KazeTap { float *kc; long *hist; float *Lt, *Lsmooth, *Lflow, *Ldet; KazeLists *lists; };
int detect_kaze_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_kaze_params &par, std::vector<modsx_keypoint> *out);
int debug_kaze(modsx_ctx *c, const modsx_image *img, const modsx_kaze_params &par, const KazeTap &tap);
int debug_kaze_scan(modsx_ctx *c, int rows, int cols, const modsx_kaze_params &par, const float *ldet, KazeLists &lists);
// DAISY (engine_daisy.hip).  patches [n][41][41] f32 / desc [n][(radq * thq + 1) * 8] f32: host pointers, or device pointers
// (4-byte aligned) when onDevice.  daisy_check_args: the refusals that need no device (patchSize, rad, radq, thq, histq, nrmType),
// made by the entries of capi.hip before they call in here; fn names the entry in the error text
int daisy_check_args(const char *fn, int patchSize, int rad, int radq, int thq, int histq, int nrmType);
int daisy_dim(int radq, int thq, int histq);
int daisy_tables(int rad, int radq, int thq, int histq, float *k5, float *kos8, float *zin8, int *fsz, float *taps, int *selected,
                 int *state, int *base, float *w);
int daisy_patches(modsx_ctx *c, const float *patches, int n, int rad, int radq, int thq, int nrmType, float *desc, bool onDevice);
int describe_regions_daisy(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                           int photoNorm, int rad, int radq, int thq, int nrmType, float *desc, bool onDevice);
int set_vs_pars(const double *scale_set, int ns, const double *tilt_set, int nt, double phi_base, double InitSigma,
                int doBlur, modsx_view *par, int cap, modsx_view *prev, int *nprev, int cap_prev);
// slot < 0: the view is a fresh allocation owned by the returned image (public API).  slot in [0, MAXB): the view lives in
// the context's pooled buffer `slot`, nothing is allocated or freed and the call does not synchronise the stream (the
// per-view loop: hipMalloc / hipFree synchronise the whole device, i.e. every other context's stream as well).
int synth_view(modsx_ctx *c, const modsx_image *gray, const modsx_view &v, modsx_image **out, double *H, int *identity,
               int slot = -1);
// n <= MAXB (image, view) items synthesised as one launch set (modsx_debug_synth_views); out[i] owns its pixels unless identity[i]
int synth_views_set(modsx_ctx *c, const modsx_image *const *grays, const modsx_view *views, int n, modsx_image **out, int *identity);
// views that took the fused kernel, the groups of shared rotations they formed, the pixels those groups rotate: every context
// of the process since the last reset (modsx_debug_views_counters).  MODSX_VIEWS_SHARE_ROT=0: every view a group of its own.
void views_counters(unsigned long long *viewsFused, unsigned long long *groups, unsigned long long *rotPx, bool reset);
bool views_share_rotation();
// the per-view loop over (source image, view) items: one launch set may mix the views of several images
int detect_describe_items(modsx_ctx *c, const modsx_image *const *itemImg, const int *itemView, int nitems, const modsx_view *views,
                          const modsx_pair_params &pp, std::vector<modsx_region> &regs,
                          float *devF, uint8_t *devU8, size_t devCapRegions, float *hostDesc, int *itemCounts,
                          const DescSet *ds = nullptr, uint8_t *const *devU8x = nullptr);
int detect_describe_views(modsx_ctx *c, const modsx_image *gray, const modsx_view *views, int nv,
                          const modsx_pair_params &pp, int view_begin, int view_step, std::vector<modsx_region> &regs,
                          float *devF, uint8_t *devU8, size_t devCapRegions, float *hostDesc, int *viewCounts,
                          const DescSet *ds = nullptr, uint8_t *const *devU8x = nullptr);
// One image's side of a (detector, descriptor) class -- RegionVectorMap[det][desc] of one ImageRepresentation: the accumulated
// regions, the device buffer of their [n][128] u8 descriptors and its capacity in regions.  The fused callers keep these in a
// context's scratch for one call (engine_views.hip LadderClass), a stored representation owns them (engine_reps.hip).
struct ClassSide { std::vector<modsx_region> *regs; size_t *cap; DevBuf *buf; };
int class_side_reserve(modsx_ctx *c, const ClassSide &k, size_t keepRows);   // room for *k.cap regions, the first keepRows kept
// SynthDetectDescribeKeypoints + AddRegions of one step for one image: ks[j] = the side of the step's j-th descriptor class
int accumulate_views(modsx_ctx *c, const ClassSide *ks, const DescSet &ds, const modsx_image *img, const modsx_view *views, int nv,
                     const modsx_pair_params &pp, modsx_comm *cm = nullptr, bool split = false);
void ctx_worker_stop(modsx_ctx *c);   // joins the context's host thread, if it has one (ctx_destroy)
void rebase_ids(std::vector<modsx_region> &regs, const int *viewCounts, int nv, size_t base);
struct VerifyTask;
// defer != nullptr (one-step ladders only): the tentatives are matched and handed back unverified
int match_ladder(modsx_ctx *c, const modsx_image *img1, const modsx_image *img2, const modsx_ladder_step *steps, int nsteps,
                 int min_matches, const modsx_pair_params &pp, modsx_pair_result *res, int *steps_done, VerifyTask *defer = nullptr,
                 modsx_comm *comm = nullptr, int owner = -1);
int match_pair_views(modsx_ctx *c, const modsx_image *img1, const modsx_image *img2, const modsx_view *views, int nv,
                     const modsx_pair_params &pp, modsx_pair_result *res, VerifyTask *defer = nullptr);
// per-kernel-class GPU timing with HIP events on the launch stream (engine.hip); *slot = (size_t)-1 when profiling is off
void prof_begin(modsx_ctx *c, int cls, double work, size_t *slot);
void prof_end(modsx_ctx *c, size_t slot);
bool prof_reserve(modsx_ctx *c, int cls, double work, hipEvent_t *ev2);
struct ProfScope {     // prof_begin ... prof_end around the launches of a block
  modsx_ctx *c;
  size_t slot;
  ProfScope(modsx_ctx *c_, int cls, double work) : c(c_) { prof_begin(c, cls, work, &slot); }
  ~ProfScope() { prof_end(c, slot); }
  ProfScope(const ProfScope &) = delete;
  ProfScope &operator=(const ProfScope &) = delete;
};
// MODSX_HOST_TIMING=2: wall time of the host phases between the launches of a set (stderr)
struct HostMark {
  bool on; double t;
  HostMark() : on(getenv("MODSX_HOST_TIMING") && atoi(getenv("MODSX_HOST_TIMING")) >= 2), t(0) { if (on) t = now(); }
  static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void mark(const char *what) { if (!on) return; const double n = now(); fprintf(stderr, "  host %-28s %.3f ms\n", what, n - t); t = n; }
};
inline double now_ms() { return HostMark::now(); }
inline size_t align_up(size_t bytes, size_t a) { return (bytes + a - 1) & ~(a - 1); }   // a: a power of two
// a list handed over the C ABI as a malloc'd array (never of size 0); the caller frees it
template <typename T>
inline T *to_malloc(const std::vector<T> &v) {
  T *p = (T *)malloc(sizeof(T) * (v.size() ? v.size() : 1));
  if (p && !v.empty()) memcpy(p, v.data(), sizeof(T) * v.size());
  return p;
}
// Stable LSD radix sort of w by its bits loBit..hiBit, 11 bits per pass; a pass whose digit is the same in every word is left
// out.  tmp is the second buffer of the passes (resized here; callers keep it to keep its memory).
inline void host_radix_sort_u64(std::vector<uint64_t> &w, std::vector<uint64_t> &tmp, int loBit, int hiBit) {
  constexpr int BITS = 11, NB = 1 << BITS;
  const size_t m = w.size();
  if (!m) return;
  tmp.resize(m);
  uint32_t hist[NB];
  for (int shift = loBit; shift <= hiBit; shift += BITS) {
    memset(hist, 0, sizeof hist);
    for (size_t k = 0; k < m; k++) hist[(w[k] >> shift) & (NB - 1)]++;
    if (hist[(w[0] >> shift) & (NB - 1)] == m) continue;
    uint32_t sum = 0;
    for (int b = 0; b < NB; b++) { const uint32_t h = hist[b]; hist[b] = sum; sum += h; }
    for (size_t k = 0; k < m; k++) tmp[hist[(w[k] >> shift) & (NB - 1)]++] = w[k];
    w.swap(tmp);
  }
}
// a sharded match (engine_shard.hip): this rank owns the query rows [lo, lo + per) of n1_total
struct MatchShard { void *comm; int world, per, n1_total, lo; };
// the lane's (per + 1)-row blocks (header row + result rows), grown by agreement; then header + all-gather + download + wait
int match_shard_begin(modsx_ctx *c, const MatchShard &sh, mx::MatchRow **blk);
int match_shard_gather(modsx_ctx *c, const MatchShard &sh, int local_rc, mx::MatchRow *host);
int detect_describe_views_sharded(modsx_ctx *c, modsx_comm *cm, const modsx_image *img, const modsx_view *views, int nv,
                                  const modsx_pair_params &pp, const DescSet &ds, std::vector<modsx_region> &regs,
                                  DevBuf *const *descAcc, const size_t *base, int *viewCounts);
int detect_describe_items_sharded(modsx_ctx *c, modsx_comm *cm, const modsx_image *const *imgs, int nimg, const modsx_view *views,
                                  int nviews, const modsx_pair_params &pp, const DescSet &ds, std::vector<modsx_region> &regs,
                                  DevBuf *const *descAcc, const size_t *base, int *itemCounts, const unsigned char *wantImg = nullptr,
                                  std::vector<size_t> *regStart = nullptr, double **devPos = nullptr, std::vector<double> *kpRows = nullptr,
                                  const int *ownerImg = nullptr);   // ownerImg[j]: the one rank that reads image j's rows (owner-only exchange)
void rows_to_tentatives(const MatchRow *rows, int n1, int nn, std::vector<modsx_tentative> &o, const int *ddb = nullptr,
                        double sqminratio = 0, std::vector<double> *d2byDB = nullptr);
int comm_rank(const modsx_comm *cm);
int comm_world(const modsx_comm *cm);
int comm_same_value(modsx_ctx *c, modsx_comm *cm, int value, const char *what);   // one 4-byte all-gather; an error on every rank when they differ
int match_sharded(modsx_ctx *c, modsx_comm *cm, const uint8_t *d1, int n1, const uint8_t *d2, int n2, const double *pos2Host,
                  double ratioT, double contradDist, int nn, std::vector<modsx_tentative> &out);
int match_device_batch(modsx_ctx *c, int nb, const uint8_t *const *d1, const int *n1, const uint8_t *const *d2, const int *n2,
                       const double *const *pos2Host, double ratioT, double contradDist, int nn,
                       std::vector<modsx_tentative> *out, const MatchShard *shard, const double *const *pos2Dev = nullptr,
                       const DbSet *db = nullptr, std::vector<double> *d2byDB = nullptr,    // db: MatchFlannFGINNPlusDB; d2byDB[i] aligned with out[i]
                       const void *const *trainPack = nullptr);                             // trainPack[i]: problem i's trains are pre-packed there
int match_device(modsx_ctx *c, const uint8_t *d1, int n1, const uint8_t *d2, int n2, const double *pos2Host,
                 double ratioT, double contradDist, int nn, std::vector<modsx_tentative> &out, const DbSet *db = nullptr,
                 std::vector<double> *d2byDB = nullptr);
int match_host_desc(modsx_ctx *c, const float *desc1, int n1, const float *desc2, int n2, const double *pos2,
                    double ratioT, double contradDist, int nn, std::vector<modsx_tentative> &out, const DbSet *db = nullptr,
                    std::vector<double> *d2byDB = nullptr);
// ---- MatchFLANNDistance, exact Hamming search (engine_hamming.hip) ----
int hamming_tentatives(const int *nn2, int n1, double distanceThreshold, std::vector<modsx_tentative> &out);   // the record rule (host)
int hamming_check_args(const char *fn, int n1, int n2, int nbytes);
int hamming_search_device(modsx_ctx *c, const uint8_t *d1, int n1, const uint8_t *d2, int n2, int nbytes, int splits, int *nn2, int *geo4);
int match_hamming_device(modsx_ctx *c, const uint8_t *d1, int n1, const uint8_t *d2, int n2, int nbytes, double distanceThreshold,
                         std::vector<modsx_tentative> &out);
int match_hamming_host(modsx_ctx *c, const void *desc1, int n1, const void *desc2, int n2, int nbytes, int dtype, double distanceThreshold,
                       std::vector<modsx_tentative> &out);
int match_regions_hamming(modsx_ctx *c, const modsx_region *regs1, const void *desc1, int n1, const modsx_region *regs2, const void *desc2,
                          int n2, int nbytes, int dtype, double distanceThreshold, const modsx_pair_params &pp, modsx_pair_result *res);
// ---- MatchFlannFGINN on f32 rows of any width (engine_fginn32.hip; the host's walk, its records and fginn32_dpass: fginn_walk.hpp) ----
// debug tap: splits forces the split count (0 = production); stageMask: 1 = top-4 + host walk (always run), 2 = k_f32_resolve
// (a query that needs a stage that is masked off gives no record).  Outputs (each optional): top4 [n1][4] keys, stage [n1] = how
// the query was closed (0 host walk, 1 resolve sweep, 2 resolve sweep and its count: the rank bound exceeded nn - 1), geometry [6],
// counters [4] = {queries sent to resolve, of those closed by the count, records, validity flag}
struct Fginn32Tap { int splits, stageMask; unsigned long long *top4; unsigned char *stage; int *geometry; int *counters; };
bool fginn32_rows_ok(const float *f, size_t n);     // every value finite with |x| <= 1e17
int fginn32_check_args(const char *fn, int n1, int n2, int dim, double ratioT, int nn);
int fginn32_check_dist(const char *fn, int dist);   // MODSX_DIST_L2 or MODSX_DIST_L1
int fginn32_geometry_report(int n1, int n2, int dim, int splits, int *geo6);
int fginn_l1_geometry_report(int n1, int n2, int splits, int *geo6);
// dist: the chain of the sweep (MODSX_DIST_L2 / MODSX_DIST_L1; the host entries check it, the device entry's caller does)
int match_fginn32_device(modsx_ctx *c, const float *d1, int n1, const float *d2, int n2, int dim, const double *pos2, double ratioT,
                         double contradDist, int nn, std::vector<modsx_tentative> &out, const Fginn32Tap *tap = nullptr, int dist = MODSX_DIST_L2);
int match_fginn32_host(modsx_ctx *c, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2, double ratioT,
                       double contradDist, int nn, std::vector<modsx_tentative> &out, const Fginn32Tap *tap = nullptr, int dist = MODSX_DIST_L2);
int match_regions_f32(modsx_ctx *c, const modsx_region *regs1, const float *desc1, int n1, const modsx_region *regs2, const float *desc2,
                      int n2, int dim, const modsx_pair_params &pp, modsx_pair_result *res, int dist = MODSX_DIST_L2, bool bytes = false);
// L1 on rows holding the integers 0..255 at 128 columns, searched as bytes (kernels_fginn_l1.hip): dense [n][128] u8 rows in HBM of
// any alignment, or [n][128] f32 rows from the host (anything but those integers is refused)
int match_fginn_l1_device(modsx_ctx *c, const uint8_t *d1, int n1, const uint8_t *d2, int n2, const double *pos2, double ratioT,
                          double contradDist, int nn, std::vector<modsx_tentative> &out, const Fginn32Tap *tap = nullptr);
int match_fginn_l1_host(modsx_ctx *c, const float *desc1, int n1, const float *desc2, int n2, const double *pos2, double ratioT,
                        double contradDist, int nn, std::vector<modsx_tentative> &out, const Fginn32Tap *tap = nullptr);
DbSet *db_create(modsx_ctx *c, const void *rows, long n, int dtype);
void db_free(DbSet *db);
int db_nearest(modsx_ctx *c, const DbSet &db, const float *desc, int n, float *dmin);
// MatchImgReps (correspondencebank.cpp:333-341): with useDBforFGINN the RootSIFT classes, and no other, are matched against the database
inline const DbSet *fginn_db_for(const modsx_ctx *c, int descType) { return descType == MODSX_DESC_ROOT_SIFT ? c->fginnDb : nullptr; }
// The region list a tentative's indices refer to: the per-class lists of one image in the order GetCorresponcesVector walks
// the classes (descriptor name, then detector name), as segments -- two descriptor classes of one detector share their
// regions, so the concatenation is never materialised.
constexpr int REP_CLASSES_MAX = 2 * MODSX_MAX_DESC + 3 * 5 + 4 * 3;   // the u8, the float and the binary classes of a stored representation
struct RegList {
  const modsx_region *p[REP_CLASSES_MAX];
  size_t end[REP_CLASSES_MAX];   // running end index of every segment
  int n = 0;
  void clear() { n = 0; }
  void add(const modsx_region *q, size_t cnt) { p[n] = q; end[n] = (n ? end[n - 1] : 0) + cnt; n++; }
  void add(const std::vector<modsx_region> &v) { add(v.data(), v.size()); }
  size_t size() const { return n ? end[n - 1] : 0; }
  const modsx_region &operator[](size_t i) const {
    int k = 0;
    while (k < n - 1 && i >= end[k]) k++;     // an index past size() is a caller bug: it lands in the last segment and trips the check
    if (i >= end[k]) abort();
    return p[k][i - (k ? end[k - 1] : 0)];
  }
};
void verify_tentatives(const RegList &r1, const RegList &r2, const std::vector<modsx_tentative> &tents,
                       const modsx_pair_params &pp, modsx_pair_result *res);
void verify_tentatives(const std::vector<modsx_region> &r1, const std::vector<modsx_region> &r2,
                       const std::vector<modsx_tentative> &tents, const modsx_pair_params &pp, modsx_pair_result *res);
void verify_tentatives_kp(const double *kp1, size_t n1, const double *kp2, size_t n2, const std::vector<modsx_tentative> &tents,
                          const modsx_pair_params &pp, modsx_pair_result *res);
// ---- the host plumbing the exact searches share (Hamming, f32 / byte-row FGINN, single and grouped) ----
// The search round trip: launch(ev) issues the search on c->stream (ev: three events to record before the packing, behind it and
// behind the search, or null); `bytes` of its result come down from dev to the pinned host buffer.  ms (null: never timed) receives
// the two event intervals under modsx_profile.  The events are destroyed on the error path too.
template <class L>
int search_download(modsx_ctx *c, L &&launch, const void *dev, void *host, size_t bytes, double *ms) {
  hipEvent_t ev[3];
  const bool timed = ms && c->prof.enabled;     // modsx_profile: the launches are timed into the context, no new kernel class
  if (timed) for (int i = 0; i < 3; i++) MX_HIP(hipEventCreate(&ev[i]));
  launch(timed ? ev : nullptr);
  hipError_t e = ctx_copy(c, host, dev, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = ctx_sync(c);
  if (e == hipSuccess) e = hipGetLastError();
  if (timed) {
    float a = 0, b = 0;
    if (e == hipSuccess && hipEventElapsedTime(&a, ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev[1], ev[2]) == hipSuccess) {
      ms[0] = a; ms[1] = b;
    }
    for (int i = 0; i < 3; i++) hipEventDestroy(ev[i]);
  }
  MX_HIP(e);
  return MODSX_OK;
}
// The resolve round trip of the FGINN walk: open[] and the initial closed[] = {all ones, 0} up to dOpen / dClosed, launch() (the
// resolve sweep on c->stream), closed[] down.  Pageable memory on both ends, so it ends with a stream synchronisation.
template <class L>
int resolve_round_trip(modsx_ctx *c, const std::vector<F32Open> &open, F32Open *dOpen, F32Closed *dClosed, std::vector<F32Closed> &closed,
                       L &&launch) {
  const size_t nu = open.size();
  closed.assign(nu, F32Closed{KEY_NONE, 0u, 0u});
  MX_HIP(hipMemcpyAsync(dOpen, open.data(), nu * sizeof(F32Open), hipMemcpyHostToDevice, c->stream));
  MX_HIP(hipMemcpyAsync(dClosed, closed.data(), nu * sizeof(F32Closed), hipMemcpyHostToDevice, c->stream));
  launch();
  MX_HIP(hipMemcpyAsync(closed.data(), dClosed, nu * sizeof(F32Closed), hipMemcpyDeviceToHost, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}
// two pageable host row sets into a pair of context buffers; synchronised, so the sources may be temporaries (engine_hamming.hip)
int upload_row_pair(modsx_ctx *c, DevBuf *buf2, const void *rows1, size_t bytes1, const void *rows2, size_t bytes2);
// What the match_regions_* entries have in common: the zeroed result with H = -1 (all an empty side or an error leaves), then
// match(tents) -- the caller's argument checks, before any work, and its search -- then DuplicateFiltering + LORANSACFiltering of
// the tentatives on the two caller-supplied region lists.
template <class M>
int match_regions_with(const modsx_region *regs1, int n1, const modsx_region *regs2, int n2, const modsx_pair_params &pp,
                       modsx_pair_result *res, M &&match) {
  memset(res, 0, sizeof *res);
  for (int i = 0; i < 9; i++) res->H[i] = -1;
  std::vector<modsx_tentative> tents;
  const int rc = match(tents);
  if (rc) return rc;
  res->n_regions1 = n1; res->n_regions2 = n2;
  if (n1 == 0 || n2 == 0) return MODSX_OK;
  RegList l1, l2;
  l1.add(regs1, (size_t)n1); l2.add(regs2, (size_t)n2);
  verify_tentatives(l1, l2, tents, pp, res);
  return MODSX_OK;
}
// A pair whose tentatives are matched but not yet verified: modsx_match_pairs hands these to helper threads so that a
// context's stream is fed the next group while the host runs DuplicateFiltering + LO-RANSAC of this one.  The task owns the
// region vectors its two lists point into (moving a vector keeps its heap block, so the segments stay valid).
struct VerifyTask {
  std::vector<std::vector<modsx_region>> own;
  RegList l1, l2;
  std::vector<modsx_tentative> tents;
  modsx_pair_result *res = nullptr;
  int dev = 0;        // the device of the context that produced the task: the verifier's device-side loops (rFtH counting) run there
  VerifyTask() = default;
  VerifyTask(VerifyTask &&) = default;
  VerifyTask &operator=(VerifyTask &&) = default;
  VerifyTask(const VerifyTask &) = delete;              // l1 / l2 point into `own`: a copy would dangle
  VerifyTask &operator=(const VerifyTask &) = delete;
};
// deferred == nullptr: verification runs inline, pair by pair.  Otherwise the G matching problems share the matcher's
// launches and one VerifyTask per pair is appended to *deferred instead of being verified.
// ---- stored image representations (engine_reps.hip) ----
// One (detector, descriptor) class of a stored representation: RegionVectorMap[det][desc].  `pack` is the train side of a
// matcher workspace for exactly regs.size() descriptors and the regions' reproj_kp positions (kernels_match.hip).
struct RepSlot {
  std::vector<modsx_region> regs;
  size_t cap = (size_t)1 << 16;     // regions `desc` has room for (grows x4)
  DevBuf desc, pack;
};
// What the float and the binary slot are (the store: engine_reps.hip slot_*): the host region list and the rows in their matcher's
// form -- W 4-byte words per row, zero behind the row's own width, zero rows up to the capacity (4096 x 4^k rows: whole workgroups
// of queries and whole tiles of trains at every tile length), so nothing is packed when a slot is matched and an append only
// writes behind the old rows.  A class that holds regions has capW == its W, an empty one has no buffer.
struct RepRows {
  std::vector<modsx_region> regs;
  int W = 0;
  size_t cap = 0;                // rows the buffers have room for, each of capW words
  int capW = 0;
  DevBuf rows, pos;              // pos: the regions' reproj_kp as [cap][2] f64, float slots only
};
// One float class (engine_reps_f32.hip): rows as kernels_fginn32.hip takes them, W = DK floats.  dim is fixed by the first append
// that succeeds.  The first capacity is MODSX_REP_F32_FIRST_ROWS, that of a binary slot MODSX_REP_BIN_FIRST_ROWS.
struct RepSlotF : RepRows {
  std::vector<double> hpos;      // reproj_kp.x, y of regs, dense: what the host's walk reads
  int dim = 0;
};
// One binary class (engine_reps_bin.hip): rows exactly as k_hamming_pack writes them (kernels_hamming.hip), W = WK dwords.  nbytes
// is fixed by the first append that succeeds.
struct RepSlotB : RepRows { int nbytes = 0; };
void slot_release(RepRows &k);
// room for `rows` rows of W words: the old rows (and positions, isFloat) are copied once, everything behind them is zero
int slot_reserve(modsx_ctx *c, RepRows &k, size_t rows, int W, bool isFloat);
hipError_t slot_zero_again(modsx_ctx *c, RepRows &k, size_t base, int n);      // rows base .. base + n back to zero rows, waited for
// modsx_rep_class_f32 / _bin: the regions and the rows as dense [n][widthBytes] (each optional), malloc'd; returns n
int slot_download(modsx_ctx *c, const char *fn, const RepRows &k, size_t widthBytes, modsx_region **regs, void **rows);
// The classes a representation can hold: what GetCorresponcesVector("All", "All") (correspondencebank.cpp:117-179) iterates over,
// as the one table in engine_reps.hip.  kind: which slots hold the class; det: its slot index inside the kind (u8: HessianAffine,
// MSER; float: HessianAffine, MSER, SURF; binary: HessianAffine, MSER, ORB, SURF); type = MODSX_DESC_*; order: its place in that
// iteration, 4 * (place of the descriptor name) + (place of the detector name), both in std::map order.
enum { REP_U8 = 0, REP_F32 = 1, REP_BIN = 2 };
constexpr int REP_ORDERS = 12 * 4;
struct RepClassId { int kind, det, type, order; };
bool rep_class_id(int detector, int desc_type, RepClassId *id);      // false: the pair names no class
int rep_class_detector(const RepClassId &k);                         // MODSX_DET_*
inline bool rep_class_of_kind(int detector, int desc_type, int kind, int *det) {
  RepClassId k;
  if (!rep_class_id(detector, desc_type, &k) || k.kind != kind) return false;
  *det = k.det;
  return true;
}
inline bool rep_class_ok(int detector, int desc_type, int *det) { return rep_class_of_kind(detector, desc_type, REP_U8, det); }
inline bool rep_class_f32_ok(int detector, int desc_type, int *det) { return rep_class_of_kind(detector, desc_type, REP_F32, det); }
inline bool rep_class_bin_ok(int detector, int desc_type, int *det) { return rep_class_of_kind(detector, desc_type, REP_BIN, det); }
// the tentatives of every class's last match against one partner (CorrespondencesMapMap[desc][det]), by RepClassId::order
struct RepTents { std::vector<modsx_tentative> of[REP_ORDERS]; };
const std::vector<modsx_region> &rep_class_regions(const modsx_rep *rep, const RepClassId &k);
// sorted by order: the order GetCorresponcesVector("All", "All") concatenates the classes in
struct RepClassList {
  int n = 0;
  RepClassId k[REP_CLASSES_MAX];
  bool has(const RepClassId &c) const { for (int i = 0; i < n; i++) if (k[i].order == c.order) return true; return false; }
  void add(const RepClassId &c) {
    int at = n++;
    for (; at > 0 && k[at - 1].order > c.order; at--) k[at] = k[at - 1];
    k[at] = c;
  }
};
void rep_classes(RepClassList &l, unsigned kinds);               // every class of the kinds in the mask (1 << REP_U8 | ...)
int rep_class_rank(int detector, int desc_type);                 // modsx_rep_class_rank; -1: no such class
int rep_class_order(int detector, int desc_type);                // modsx_rep_class_order; -1: no such class
int rep_add_views(modsx_ctx *c, modsx_rep *rep, const modsx_image *img, const modsx_ladder_step &st, const modsx_pair_params &pp);
int reps_match_group(modsx_ctx *c, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, const modsx_rep_class_sel *sel, int nsel,
                     const modsx_pair_params &pp, RepTents *const *tents);
void reps_verify_task(const modsx_rep *rep1, const modsx_rep *rep2, const RepClassList &classes, const RepTents &tents,
                      modsx_pair_result *res, int dev, VerifyTask &task);
// float classes (engine_reps_f32.hip); det = the slot index rep_class_f32_ok gives
// rows: [n][dim] f32 on the host, or a device pointer (4-byte aligned) when onDevice
int rep_append_f32(modsx_ctx *c, modsx_rep *rep, int det, int type, const modsx_region *regs, const float *rows, int dim, int n,
                   bool onDevice = false);
int rep_describe_append(modsx_ctx *c, modsx_rep *rep, int det, int type, const modsx_image *img, const modsx_region *regs, int n,
                        double mrSize, int patchSize, int fast, int photoNorm, const int *daisyPar);
int rep_class_f32(modsx_ctx *c, const modsx_rep *rep, int det, int type, modsx_region **regs, float **rows, int *dim);
// MatchFlannFGINN of one float class for G <= MATCH_MAXB partners in one grouped launch set; outs[g]: partner g's records
int reps_f32_match_group(modsx_ctx *c, const char *fn, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, int det, int type,
                         double ratio, double contradDist, int nn, std::vector<modsx_tentative> *outs);
// binary classes (engine_reps_bin.hip); det = the slot index rep_class_bin_ok gives
int rep_append_bin(modsx_ctx *c, modsx_rep *rep, int det, int type, const modsx_region *regs, const uint8_t *rows, bool onDevice,
                   int nbytes, int n, const char *fn);
int rep_class_bin(modsx_ctx *c, const modsx_rep *rep, int det, int type, modsx_region **regs, unsigned char **rows, int *nbytes);
// what every stored Hamming match refuses before any launch, over n partners: another device, widths that differ, a train class
// of exactly one region, a threshold that is not positive and finite
int reps_bin_check(const char *fn, const modsx_ctx *c, const modsx_rep *rep1, const modsx_rep *const *reps2, int n, int det, int type,
                   double distanceThreshold);
// MatchFLANNDistance of one binary class for G <= MATCH_MAXB partners in one grouped launch set; outs[g]: partner g's records
int reps_bin_match_group(modsx_ctx *c, const char *fn, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, int det, int type,
                         double distanceThreshold, std::vector<modsx_tentative> *outs);
// modsx_debug_fginn32_group_geometry / modsx_debug_hamming_group_geometry: the report of an F32Group or a HamGroup of kernel width W
template <class Group>
inline int group_geometry_report(const Group &g, int W, const int *prob, int G, int total, int *geometry, int *per_problem, int *splits,
                                 int cap) {
  geometry[0] = g.tile; geometry[1] = W; geometry[2] = g.gx; geometry[3] = total;
  memset(per_problem, 0, sizeof(int) * 3 * G);
  for (int p = 0; p < g.np; p++) {
    int *o = per_problem + 3 * prob[p];
    o[0] = g.ntiles[p]; o[1] = g.S[p]; o[2] = g.tps[p];
    for (int s = 0; s < g.S[p] && g.first[p] + s < cap; s++) {
      int *sp = splits + 3 * (g.first[p] + s);
      sp[0] = prob[p]; sp[1] = s * g.tps[p]; sp[2] = std::min(g.ntiles[p], (s + 1) * g.tps[p]);
    }
  }
  return total;
}
bool desc_f32_to_u8(const float *f, size_t n, uint8_t *u);   // false: a value that is not one of the integers 0..255
int match_pair_group(modsx_ctx *c, const modsx_image *const *imgs1, const modsx_image *const *imgs2, int G,
                     const modsx_pair_params &pp, modsx_pair_result *res, std::vector<VerifyTask> *deferred = nullptr);
int match_pair(modsx_ctx *c, const modsx_image *img1, const modsx_image *img2, const modsx_pair_params &pp,
               modsx_pair_result *res);

// filters.cpp / ransac.cpp (host)
int duplicate_filtering(const double *pts, const double *key, int T, double r, int do_sort, int *order,
                        unsigned char *keep);
int ransac_h(const double *u, int len, double th, double conf, int max_sam, double *H, unsigned char *inl, int *data_out,
             int oriented_constraint, int doSymCheck, unsigned seed0, double *scoreJ, int error_type = 0);
void hds_sym(const double *u, const double *H, double *p, int len, bool takeMax);
void hds_sym_setup(const double *H, double *Hinv, double *H1);                 // hds_sym = setup + with
void hds_sym_with(const double *u, const double *Hinv, const double *H1, double *p, int len, bool takeMax);
int save_regions(const char *path, const modsx_region_class *classes, int nclasses);
int load_regions(const char *path, const char *det_name, const char *desc_name, std::vector<modsx_region> &regs,
                 std::vector<float> &desc, int *dim, std::string *found_det, std::string *found_desc);
int detect_msers_host(const uint8_t *u8, int rows, int cols, const modsx_mser_params &par, double tilt, double zoom,
                      std::vector<modsx_keypoint> &out);
// devOrder[i] / devStart[i]: view i's pixel offsets in (grey level, raster) order and the 257 level starts when the device sorted the
// view (launch_mser_sort), or null: the host sorts
int detect_msers_views(const uint8_t *const *u8, const int *rows, const int *cols, int n, const modsx_mser_params &par,
                       const double *tilts, const double *zooms, std::vector<modsx_keypoint> *out, const int *const *devOrder = nullptr,
                       const int *const *devStart = nullptr);
// engine_views.hip: u8 truncation (+ bin sort with devSort) of the n <= MAXB views of a launch set on the device and the one
// download of the block; per view the host pointers into c->hMser that detect_msers_views takes
struct MserFront { const uint8_t *u8[MAXB]; const int *order[MAXB], *start[MAXB]; };
int mser_front(modsx_ctx *c, const float *const *dview, const int *rows, const int *cols, int n, bool devSort, MserFront &out);
// fn(0) .. fn(n - 1) on the process-wide host worker pool (MODSX_HOST_THREADS, default min(hardware threads, 64)) + the caller
void host_parallel_for(int n, const std::function<void(int)> &fn, bool light = false);
void host_light_pool(bool on);   // this thread's short host loops may use the pool regardless of the sets in flight
void host_set_enter();
void host_set_leave();
inline void host_parallel_light(int n, const std::function<void(int)> &fn) { host_parallel_for(n, fn, true); }
int ransac_f(const double *u, int len, double th, double conf, int max_sam, double *F, unsigned char *inl, int *data_out,
             int do_lo, unsigned inlLimit, int error_type, int doSymCheck, unsigned seed0);
int loransac_f(const double *pts, const double *laf1, const double *laf2, int T, double err_threshold, double confidence,
               int max_samples, int lo, double LAFCoef, int doSymmCheck, int error_type, unsigned seed, double *F,
               unsigned char *inl, unsigned char *keep, int *data_out3);
int loransac_h(const double *pts, const double *laf1, const double *laf2, int T, double err_threshold,
               double confidence, int max_samples, int lo, double HLAFCoef, int doSymmCheck, unsigned seed, double *H,
               double *Hraw, unsigned char *inl, unsigned char *keep, int *data_out, int error_type = 0);
}  // namespace mx

// slot[det][type]: det 0 = HessianAffine, 1 = MSER; type = MODSX_DESC_* 0..3.  fslot[det][type - MODSX_DESC_CAFFE]: det 2 = SURF.
// bslot[det][type - MODSX_DESC_BRISK]: det 0 = HessianAffine, 1 = MSER, 2 = ORB, 3 = SURF
struct modsx_rep { int dev; mx::RepSlot slot[2][4]; mx::RepSlotF fslot[3][5]; mx::RepSlotB bslot[4][3]; };
